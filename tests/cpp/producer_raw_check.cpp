// producer_raw_check.cpp -- the raw mode of the batchfile reader (bvamd::BgzfRawReader, host/batch_producer.hpp) against the
// text mode (BatchfileProducer::run_text), without a GPU.
//
//   producer_raw_check FILE[,FILE...] [REWRITE_DIR]
//
// The raw reader hands out, per file, runs of whole BGZF members from a cursor onward; the device then inflates them, finds the
// lines, takes min(max_positions, the files' complete lines) positions and returns the cursors of the first lines not taken
// (bv_engine_text_parse_bgzf).  Here a CPU stand-in plays the device -- zlib inflates each run, the lines are cut with memchr --
// under the same contract (skip_bytes, skip_lines, at_end, cursor = (member, offset)), and the rows of all batches, in order,
// must be the rows of run_text's blocks, row for row, over the whole files: for several run sizes and max_positions, 1 among
// them.  With REWRITE_DIR the files are also rewritten through BgzfWriter (host/bgzf_tabix.hpp: 0xff00-byte members, zlib's
// default level) and checked again.  Prints "OK ..." and exits 0, or "FAIL: ..." and exits 1.
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../basevar_amd/host/batch_producer.hpp"
#include "../../basevar_amd/host/bgzf_tabix.hpp"

namespace {

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

typedef std::vector<std::string> Rows;  // every row with its '\n', position-major

Rows text_mode(const std::vector<std::string> &files, size_t block_bytes, size_t max_positions, int threads) {
    Rows out;
    Opened in(files);
    bvamd::BatchfileProducer producer(in.readers, in.first_row, in.have_row, in.n_sample, threads);
    producer.set_paths(files, in.header_lines);
    if (producer.bgzf_files() != files.size()) throw std::runtime_error("not every file is BGZF");
    producer.run_text([&](std::string &rows, std::vector<uint64_t> &row_off, size_t n_positions) {
        for (size_t r = 0; r < n_positions * files.size(); ++r) out.emplace_back(rows, (size_t)row_off[r], (size_t)(row_off[r + 1] - row_off[r]));
        return true;
    }, block_bytes, max_positions);
    return out;
}

std::string inflate_member(const unsigned char *m, size_t total) {
    const uint32_t isize = (uint32_t)m[total - 4] | ((uint32_t)m[total - 3] << 8) | ((uint32_t)m[total - 2] << 16) | ((uint32_t)m[total - 1] << 24);
    std::string out(isize, '\0');
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) throw std::runtime_error("inflateInit2");
    zs.next_in = const_cast<Bytef *>(m + 18);
    zs.avail_in = (uInt)(total - 26);
    zs.next_out = reinterpret_cast<Bytef *>(&out[0]);
    zs.avail_out = isize;
    const int rc = inflate(&zs, Z_FINISH);
    inflateEnd(&zs);
    if (rc != Z_STREAM_END || zs.avail_out != 0) throw std::runtime_error("a member does not inflate to its ISIZE");
    return out;
}

// the stand-in for bv_engine_text_parse_bgzf over one batch of runs
Rows raw_mode(const std::vector<std::string> &files, const std::vector<size_t> &header_lines, size_t per_file_text, size_t max_positions, uint64_t *handed,
              uint64_t *passed) {
    Rows out;
    bvamd::BgzfRawReader raw;
    if (!raw.open(files, header_lines)) throw std::runtime_error("the raw reader refuses the files");
    const size_t F = files.size();
    bvamd::BgzfRawRuns r;
    for (size_t guard = 0;; ++guard) {
        if (guard > 10000000) throw std::runtime_error("the raw loop does not end");
        raw.next(r, per_file_text);
        std::vector<std::string> text(F);
        std::vector<std::vector<size_t>> isize(F);
        std::vector<std::vector<std::pair<size_t, size_t>>> lines(F);  // [begin, end) of every line behind the skip, '\n' included
        size_t P = max_positions;
        for (size_t f = 0; f < F; ++f) {
            for (uint32_t k = r.file_member[f]; k < r.file_member[f + 1]; ++k) {
                const std::string t = inflate_member(&r.data[r.member_off[k]], (size_t)(r.member_off[k + 1] - r.member_off[k]));
                isize[f].push_back(t.size());
                text[f] += t;
            }
            if (r.skip_bytes[f] > text[f].size()) throw std::runtime_error("skip_bytes beyond the run");
            size_t at = (size_t)r.skip_bytes[f], skip = r.skip_lines[f];
            if (r.at_end && text[f].size() > at && text[f].back() != '\n') text[f] += '\n';  // (the spare byte behind the run)
            while (at < text[f].size()) {
                const void *nl = std::memchr(&text[f][at], '\n', text[f].size() - at);
                if (!nl) break;
                const size_t end = (size_t)(static_cast<const char *>(nl) - text[f].data()) + 1;
                if (skip) --skip; else lines[f].emplace_back(at, end);
                at = end;
            }
            P = std::min(P, lines[f].size());
        }
        if (P == 0) {
            if (r.at_end) break;
            per_file_text *= 2;
            continue;
        }
        for (size_t p = 0; p < P; ++p)
            for (size_t f = 0; f < F; ++f) out.emplace_back(text[f], lines[f][p].first, lines[f][p].second - lines[f][p].first);
        std::vector<uint32_t> member(F), offset(F);
        for (size_t f = 0; f < F; ++f) {
            size_t len = 0;
            for (size_t s : isize[f]) len += s;
            const size_t x = std::min(lines[f][P - 1].second, len);
            size_t k = 0, base = 0;
            while (k < isize[f].size() && base + isize[f][k] <= x) base += isize[f][k++];
            member[f] = (uint32_t)k;
            offset[f] = k < isize[f].size() ? (uint32_t)(x - base) : 0u;
        }
        raw.advance(r, member.data(), offset.data());
    }
    *handed = raw.members_handed;
    *passed = raw.members_passed;
    return out;
}

int check(const std::vector<std::string> &files, const char *what) {
    std::vector<size_t> header_lines;
    {
        Opened in(files);
        header_lines = in.header_lines;
    }
    const Rows want = text_mode(files, (size_t)1 << 25, 65536, 2);
    if (want.empty()) { std::printf("FAIL: %s: run_text delivers no row\n", what); return 1; }
    for (size_t block : {(size_t)1 << 12, (size_t)1 << 16})
        for (size_t maxp : {(size_t)1, (size_t)5}) {
            if (text_mode(files, block, maxp, 3) != want) { std::printf("FAIL: %s: run_text itself differs between block sizes\n", what); return 1; }
        }
    for (size_t per_file : {(size_t)300, (size_t)5000, (size_t)70000, ((size_t)1 << 25) / files.size()})
        for (size_t maxp : {(size_t)1, (size_t)7, (size_t)65536}) {
            uint64_t handed = 0, passed = 0;
            Rows got;
            try {
                got = raw_mode(files, header_lines, per_file, maxp, &handed, &passed);
            } catch (const std::exception &ex) {
                std::printf("FAIL: %s: run size %zu, max_positions %zu: %s\n", what, per_file, maxp, ex.what());
                return 1;
            }
            if (got != want) {
                size_t k = 0;
                while (k < got.size() && k < want.size() && got[k] == want[k]) ++k;
                std::printf("FAIL: %s: run size %zu, max_positions %zu: %zu rows against run_text's %zu, first difference at row %zu\n", what, per_file, maxp,
                            got.size(), want.size(), k);
                return 1;
            }
            if (handed < passed) { std::printf("FAIL: %s: fewer members handed out than passed\n", what); return 1; }
        }
    std::printf("OK %s: %zu rows of %zu files\n", what, want.size(), files.size());
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::vector<std::string> files = bvamd::pieces(argv[1], ',');
    try {
        if (check(files, "as given")) return 1;
        if (argc > 2) {
            std::vector<std::string> again;
            for (size_t f = 0; f < files.size(); ++f) {
                gzFile in = gzopen(files[f].c_str(), "rb");
                if (!in) throw std::runtime_error("cannot open " + files[f]);
                const std::string path = std::string(argv[2]) + "/rewritten_" + std::to_string(f) + ".gz";
                bvamd::BgzfWriter w;
                w.open(path);
                char buf[1 << 16];
                for (int n; (n = gzread(in, buf, sizeof buf)) > 0;) w.write(buf, (size_t)n);
                gzclose(in);
                w.close();
                again.push_back(path);
            }
            if (check(again, "rewritten by BgzfWriter")) return 1;
        }
    } catch (const std::exception &ex) {
        std::printf("FAIL: %s\n", ex.what());
        return 1;
    }
    return 0;
}
