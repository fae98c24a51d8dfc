// producer_text_check.cpp -- the text mode of the batchfile producer (BatchfileProducer::run_text, basevar_amd/host/
// batch_producer.hpp) against the plain loop: one line from every file per position, read in order on one thread
// (src/basetype_caller.cpp:586-611).
//   producer_text_check a.gz,b.gz,...
// For 1, 2, 3 and 8 producer threads and blocks of ~4 KiB, ~64 KiB and ~64 MiB of text: every position's lines, in order, as
// the packed blocks hand them on (rows ending in '\n', offsets in order inside the block), and the run ends where the shortest
// file ends.  No row is parsed: that is the device's work.
#include <cstdio>
#include <iostream>

#include "../../basevar_amd/host/batch_producer.hpp"

struct Opened {
    std::vector<bvamd::GzLineReader> readers;
    std::vector<std::string> first_row;
    std::vector<bool> have_row;
    std::vector<size_t> header_lines;
    size_t n_sample = 0;
    explicit Opened(const std::vector<std::string> &files) : readers(files.size()), first_row(files.size()), have_row(files.size(), false), header_lines(files.size(), 0) {
        std::vector<std::string> ids;
        for (size_t b = 0; b < files.size(); ++b) {
            if (!readers[b].open(files[b])) throw std::runtime_error("cannot open " + files[b]);
            std::string line;
            while (readers[b].getline(line)) {
                if (line.empty() || line[0] != '#') { first_row[b] = line; have_row[b] = !line.empty(); header_lines[b] += line.empty() ? 1 : 0; break; }
                bvamd::parse_sample_ids(line, ids);
                ++header_lines[b];
            }
        }
        n_sample = ids.size();
    }
};

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::vector<std::string> files = bvamd::pieces(argv[1], ',');
    const size_t NB = files.size();
    // ---- the plain loop
    std::vector<std::string> want;  // position after position, file after file
    {
        Opened in(files);
        std::vector<std::string> rows(NB);
        for (;;) {
            bool eof = false;
            for (size_t b = 0; b < NB; ++b) {
                if (in.have_row[b]) { rows[b] = in.first_row[b]; in.have_row[b] = false; }
                else if (!in.readers[b].getline(rows[b])) { eof = true; break; }
            }
            if (eof) break;
            for (auto &r : rows) want.push_back(r);
        }
    }
    // ---- the text mode
    for (size_t block_bytes : {(size_t)4 << 10, (size_t)64 << 10, (size_t)64 << 20})
        for (int threads : {1, 2, 3, 8}) {
            Opened in(files);
            bvamd::BatchfileProducer producer(in.readers, in.first_row, in.have_row, in.n_sample, threads);
            producer.set_paths(files, in.header_lines);
            std::vector<std::string> got;
            std::string bad;
            size_t blocks = 0;
            try {
                producer.run_text([&](std::string &text, std::vector<uint64_t> &off, size_t n_pos) {
                    ++blocks;
                    if (off.size() != n_pos * NB + 1 || off[0] != 0 || off.back() != text.size()) bad = "block offsets";
                    for (size_t k = 0; k + 1 < off.size() && bad.empty(); ++k) {
                        if (off[k + 1] <= off[k] || text[off[k + 1] - 1] != '\n') { bad = "row " + std::to_string(k); break; }
                        got.emplace_back(text.data() + off[k], (size_t)(off[k + 1] - off[k] - 1));
                    }
                    if (blocks % 2) { std::string t; std::vector<uint64_t> o; text.swap(t); off.swap(o); }  // the sink takes every other block
                    return true;
                }, block_bytes, 1000);
            } catch (const std::exception &ex) { bad = ex.what(); }
            if (!bad.empty() || got != want) {
                std::printf("FAIL: %d threads, blocks of %zu bytes: %zu rows (%s), the plain loop %zu\n", threads, block_bytes, got.size(),
                            bad.c_str(), want.size());
                return 1;
            }
        }
    std::printf("OK %zu positions, %zu files\n", want.size() / std::max<size_t>(NB, 1), NB);
    return 0;
}
