// text_job_check.cpp -- the file-major batchfile reader (host/file_major.hpp; bv_call --files-per-pass) against the default
// producer's text mode (host/batch_producer.hpp: BatchfileProducer::run_text), without an engine: a program of its own, built
// with -fsanitize=address,undefined by tests/test_text_job_cpu.py.
//
//   text_job_check <batchfile> ...
//
// For K = 1, 2, F - 1, F, F + 3 files per pass and windows of 1, 2, 65 and "all" positions: the groups' rows, joined again
// position-major, are the rows run_text delivers, byte for byte and as many (files of unequal length end at the shortest);
// reread(p) is the window's position p; the header scan that closes every file gives the default scan's samples; and never
// are more than K batchfiles open.  Prints one line per run (K, window, threads, windows, passes, max_open) for the test to read.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../basevar_amd/host/file_major.hpp"

using namespace bvamd;

static void require(bool ok, const std::string &what) {
    if (!ok) throw std::runtime_error(what);
}

int main(int argc, char **argv) {
    try {
        std::vector<std::string> paths(argv + 1, argv + argc);
        require(!paths.empty(), "usage: text_job_check <batchfile> ...");
        const size_t F = paths.size();
        // ---- the default route: every file open, rows position-major
        BatchfileHeaders hd;
        scan_batchfile_headers(paths, hd);
        std::vector<std::string> want;  // per position: its F rows, each with its line break
        {
            BatchfileProducer producer(hd.readers, hd.first_row, hd.have_row, hd.sample_ids.size(), 3);
            producer.set_paths(paths, hd.header_lines);
            producer.run_text([&](std::string &rows, std::vector<uint64_t> &row_off, size_t n) {
                for (size_t p = 0; p < n; ++p) want.push_back(rows.substr(row_off[p * F], row_off[(p + 1) * F] - row_off[p * F]));
                return true;
            }, (size_t)1 << 16, 50);
        }
        FileMajorHeaders fh;
        scan_batchfile_headers_closing(paths, fh);
        require(fh.sample_ids == hd.sample_ids && fh.file_samples == hd.file_samples && fh.header_lines == hd.header_lines, "the closing header scan differs");
        std::printf("positions %zu files %zu\n", want.size(), F);
        std::vector<size_t> Ks{1, 2, F > 1 ? F - 1 : 1, F, F + 3};
        const size_t windows[] = {1, 2, 65, (size_t)1 << 30};
        for (size_t K : Ks)
            for (size_t W : windows)
                for (int threads : {1, 3}) {
                    FileMajorReader rd(paths, fh.header_lines, K, threads);
                    require(rd.groups() == (F + K - 1) / K, "groups");
                    std::vector<std::string> got;
                    size_t n_windows = 0;
                    for (;;) {
                        std::vector<FileMajorReader::Group> gs(rd.groups());
                        const size_t P = rd.begin(W, gs[0]);
                        if (P == 0) break;
                        for (size_t g = 1; g < rd.groups(); ++g) rd.group(g, gs[g]);
                        const size_t used = rd.used();
                        require(used <= P && P <= W, "a window larger than asked");
                        for (size_t p = 0; p < used; ++p) {
                            std::string row;
                            for (const auto &g : gs) {
                                require(g.n_positions == P && g.row_off.size() == P * g.n_files + 1 && g.row_off[P * g.n_files] == g.text.size(), "a group's shape");
                                row.append(g.text, g.row_off[p * g.n_files], g.row_off[(p + 1) * g.n_files] - g.row_off[p * g.n_files]);
                            }
                            got.push_back(row);
                        }
                        if (used && (n_windows % 7 == 0 || used < P)) {  // the window's last position, read again
                            std::string again;
                            for (const std::string &l : rd.reread(used - 1)) again += l + "\n";
                            require(again == got.back(), "reread differs from the window's rows");
                        }
                        ++n_windows;
                        rd.end();
                        if (used < P) break;
                    }
                    require(got.size() == want.size(), "K " + std::to_string(K) + " window " + std::to_string(W) + ": " + std::to_string(got.size()) +
                                                           " positions, the default route has " + std::to_string(want.size()));
                    for (size_t p = 0; p < want.size(); ++p) require(got[p] == want[p], "K " + std::to_string(K) + " window " + std::to_string(W) + ": position " + std::to_string(p) + " differs");
                    require(rd.max_open() <= K && rd.max_open() >= 1, "K " + std::to_string(K) + ": " + std::to_string(rd.max_open()) + " batchfiles were open at once");
                    std::printf("K %zu window %zu threads %d windows %zu passes %zu max_open %zu\n", K, W, threads, n_windows, rd.passes(), rd.max_open());
                }
        return 0;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "text_job_check: %s\n", ex.what());
        return 1;
    }
}
