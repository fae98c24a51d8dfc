// tabix_query_check.cpp -- the tabix index reader and its start query (basevar_amd/host/tabix_query.hpp) as a stand-alone program,
// built with AddressSanitizer + UBSan by tests/test_tabix_query_cpu.py, which holds its answers to tests/bam_py.py's read_tbi and
// to a linear scan of the inflated file.
//
//   tabix_query_check write <lines> <member_bytes> <out.gz>   the lines (NAME \t POS \t ...) through host/bgzf_tabix.hpp's
//                                                             writer and index, a member ended whenever it holds
//                                                             member_bytes of text or more ('#' lines are written and not
//                                                             indexed); writes <out.gz> and <out.gz>.tbi
//   tabix_query_check dump <index.tbi>                        names, bins with their chunks, linear entries, as text
//   tabix_query_check query <index.tbi> <queries>             per line "NAME BEG END": "U" (unknown name), "N" (nothing
//                                                             there) or "F <virtual offset>"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../basevar_amd/host/bgzf_tabix.hpp"
#include "../../basevar_amd/host/tabix_query.hpp"

int main(int argc, char **argv) {
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (mode == "write" && argc == 5) {
            std::ifstream in(argv[2], std::ios::binary);
            const size_t member = (size_t)std::strtoull(argv[3], nullptr, 10);
            const std::string out = argv[4];
            bvamd::BgzfWriter w;
            bvamd::TabixIndex idx;
            w.open(out);
            std::string line;
            size_t n = 0;
            while (std::getline(in, line)) {
                if (!line.empty() && line[0] == '#') { w.write(line + "\n"); continue; }  // a header line: written, not indexed
                const size_t t1 = line.find('\t'), t2 = line.find('\t', t1 + 1);
                if (t1 == std::string::npos || t2 == std::string::npos) throw std::runtime_error("a line without two tabs");
                const uint64_t o0 = w.tell();
                w.write(line + "\n");
                idx.add_line(line.substr(0, t1), std::stoll(line.substr(t1 + 1, t2 - t1 - 1)), o0, w.tell());
                if (w.pending() >= member) w.flush();
                ++n;
            }
            w.close();
            idx.write(out + ".tbi");
            std::cout << "wrote " << n << " lines" << std::endl;
            return 0;
        }
        if (mode == "dump" && argc == 3) {
            bvamd::TabixReader t;
            if (!t.load(argv[2])) throw std::runtime_error("no such index");
            std::cout << "CONF";
            for (int i = 0; i < 6; ++i) std::cout << " " << t.conf()[i];
            std::cout << "\n";
            for (size_t r = 0; r < t.names().size(); ++r) {
                std::cout << "NAME " << t.names()[r] << "\n";
                for (const auto &b : t.refs()[r].bins) {
                    std::cout << "BIN " << b.first << " " << b.second.size() << "\n";
                    for (const auto &c : b.second) std::cout << "CHUNK " << c.first << " " << c.second << "\n";
                }
                std::cout << "LINEAR " << t.refs()[r].linear.size() << "\n";
                for (uint64_t o : t.refs()[r].linear) std::cout << "AT " << o << "\n";
            }
            return 0;
        }
        if (mode == "query" && argc == 4) {
            bvamd::TabixReader t;
            if (!t.load(argv[2])) throw std::runtime_error("no such index");
            std::ifstream in(argv[3]);
            std::string name;
            long long beg, end;
            while (in >> name >> beg >> end) {
                uint64_t voff = 0;
                const bvamd::TabixReader::Hit h = t.query(name, beg, end, &voff);
                if (h == bvamd::TabixReader::UNKNOWN_NAME) std::cout << "U\n";
                else if (h == bvamd::TabixReader::NOTHING) std::cout << "N\n";
                else std::cout << "F " << voff << "\n";
            }
            return 0;
        }
        std::cerr << "usage: tabix_query_check write|dump|query ..." << std::endl;
        return 2;
    } catch (const std::exception &ex) {
        std::cerr << "tabix_query_check: " << ex.what() << std::endl;
        return 1;
    }
}
