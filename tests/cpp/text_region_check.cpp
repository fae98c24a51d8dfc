// text_region_check.cpp -- the core of the region selection (basevar_amd/csrc/bv_text_region_core.h) compiled with g++ and walked
// the way the kernels of bv_text.hip walk it: tiles of <tile> bytes from skip_bytes, steps of 64 bytes, the line behind a line
// break classified in the line break's step, a step of its own for the run's first line.  tests/test_text_region_cpu.py writes
// the cases, runs this under AddressSanitizer + UBSan (every run is copied into a buffer of exactly its bytes, so a head read
// beyond the run is caught) and holds the answers to tests/text_region_model.py.
//
//   text_region_check <tile> <cases> <answers>
// cases:   CASE <F> <at_end> <cap> <beg> <end> <name_len>\n<name>\n  then F times  FILE <skip_bytes> <skip_lines> <len>\n<bytes>\n
// answers: one line per case: P done err err_file err_line err_file2, then per file n_lines first n_in term cursor
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../basevar_amd/csrc/bv_text_region_core.h"

namespace {

struct Run {
    std::vector<char> bytes;  // the run, and the spare line break where it ends an unterminated last line
    uint64_t len = 0, skip = 0, end = 0;
    uint32_t skip_lines = 0;
};

void die(const char *what) {
    std::fprintf(stderr, "text_region_check: %s\n", what);
    std::exit(2);
}

bv_tr_file walk_file(const Run &r, const bv_tr_region &rg, uint64_t tile_bytes) {
    bv_tr_file s = bv_tr_file_init();
    uint32_t breaks = 0;
    if (r.len <= r.skip) {
        bv_tr_file_finish(s, 0, r.skip_lines);
        return s;
    }
    const char *run = r.bytes.data();
    bool first_tile = true;
    for (uint64_t lo = r.skip; lo < r.end; lo += tile_bytes, first_tile = false) {
        const uint64_t hi = lo + tile_bytes < r.end ? lo + tile_bytes : r.end;
        bv_tr_tile t = bv_tr_tile_init();
        const uint32_t pre = breaks;
        uint32_t ord = pre, pos = 0;
        if (first_tile && r.skip_lines == 0) {
            const uint32_t c = bv_tr_head(run + r.skip, r.end - r.skip, rg, &pos);
            bv_tr_step(t, 1ull, (c & BV_TR_REACHED) ? 1ull : 0ull, (c & BV_TR_IN) ? 0ull : 1ull, (c & BV_TR_MAL) ? 1ull : 0ull, 0u);
        }
        for (uint64_t x0 = lo; x0 < hi; x0 += 64) {
            uint64_t B = 0, LS = 0, RE = 0, NI = 0, MA = 0;
            for (uint32_t k = 0; k < 64 && x0 + k < hi; ++k)
                if (run[x0 + k] == '\n') B |= 1ull << k;
            for (uint32_t k = 0; k < 64; ++k) {
                if (!((B >> k) & 1ull)) continue;
                if (ord + bv_tr_popc(B & bv_tr_below(k)) + 1u < r.skip_lines) continue;
                const uint64_t x = x0 + k;
                const uint32_t c = bv_tr_head(run + x + 1, r.end - (x + 1), rg, &pos);
                LS |= 1ull << k;
                if (c & BV_TR_REACHED) RE |= 1ull << k;
                if (!(c & BV_TR_IN)) NI |= 1ull << k;
                if (c & BV_TR_MAL) MA |= 1ull << k;
            }
            if (LS) bv_tr_step(t, LS, RE, NI, MA, ord + bv_tr_popc(B & bv_tr_below(bv_tr_low(LS))) + 1u - r.skip_lines);
            ord += bv_tr_popc(B);
        }
        t.cnt = ord - pre;
        breaks = ord;
        bv_tr_file_add(s, t);
    }
    bv_tr_file_finish(s, breaks, r.skip_lines);
    return s;
}

// begin of the line with raw number `raw` (line breaks of the run before it), as the scatter finds it
uint64_t line_begin(const Run &r, uint64_t raw) {
    if (raw == 0) return r.skip;
    uint64_t seen = 0;
    for (uint64_t x = r.skip; x < r.end; ++x)
        if (r.bytes[x] == '\n' && ++seen == raw) return x + 1;
    die("a taken line has no begin");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) die("usage: text_region_check <tile> <cases> <answers>");
    const uint64_t tile_bytes = std::strtoull(argv[1], nullptr, 10);
    if (tile_bytes == 0) die("tile must be > 0");
    FILE *in = std::fopen(argv[2], "rb"), *out = std::fopen(argv[3], "w");
    if (!in || !out) die("cannot open the files");
    unsigned F, at_end, cap, beg, end, name_len;
    size_t n_cases = 0;
    while (std::fscanf(in, "CASE %u %u %u %u %u %u", &F, &at_end, &cap, &beg, &end, &name_len) == 6) {
        if (std::fgetc(in) != '\n') die("bad CASE line");
        std::vector<char> name(name_len ? name_len : 1);
        if (name_len && std::fread(name.data(), 1, name_len, in) != name_len) die("short name");
        if (std::fgetc(in) != '\n') die("no line break behind the name");
        const bv_tr_region rg{name.data(), name_len, beg, end};
        std::vector<Run> runs(F);
        std::vector<bv_tr_file> files(F);
        for (unsigned f = 0; f < F; ++f) {
            unsigned long long skip, len;
            unsigned skip_lines;
            if (std::fscanf(in, "FILE %llu %u %llu", &skip, &skip_lines, &len) != 3 || std::fgetc(in) != '\n') die("bad FILE line");
            Run &r = runs[f];
            r.len = len; r.skip = skip; r.skip_lines = skip_lines;
            if (skip > len) die("skip_bytes beyond the run");
            std::vector<char> raw(len ? len : 1);
            if (len && std::fread(raw.data(), 1, len, in) != len) die("short run");
            if (std::fgetc(in) != '\n') die("no line break behind the run");
            const bool spare = at_end && len > skip && raw[len - 1] != '\n';
            r.end = len + (spare ? 1 : 0);
            r.bytes.assign(raw.begin(), raw.begin() + len);  // exactly the run's bytes ...
            if (spare) r.bytes.push_back('\n');              // ... and the spare line break
            r.bytes.shrink_to_fit();
            files[f] = walk_file(r, rg, tile_bytes);
        }
        bv_tr_result res = bv_tr_decide(files.data(), F, cap, at_end);
        // POS of the taken rows against file 0's, lowest position first
        std::vector<uint64_t> cursor(F);
        for (unsigned f = 0; f < F; ++f) cursor[f] = runs[f].skip;
        if (!res.err) {
            const bv_tr_region any{nullptr, 0, 0, 0};
            for (uint32_t p = 0; p < res.P && !res.err; ++p) {
                uint32_t pos0 = 0;
                const uint64_t b0 = line_begin(runs[0], (uint64_t)runs[0].skip_lines + files[0].first + p);
                (void)bv_tr_head(runs[0].bytes.data() + b0, runs[0].end - b0, any, &pos0);
                for (unsigned f = 1; f < F; ++f) {
                    uint32_t pos = 0;
                    const uint64_t b = line_begin(runs[f], (uint64_t)runs[f].skip_lines + files[f].first + p);
                    (void)bv_tr_head(runs[f].bytes.data() + b, runs[f].end - b, any, &pos);
                    if (pos != pos0) {
                        res.err = BV_TR_ERR_POS; res.err_file = f; res.err_line = p; res.err_file2 = 0; res.P = 0; res.done = 0;
                        break;
                    }
                }
            }
        }
        if (!res.err)
            for (unsigned f = 0; f < F; ++f)
                if (files[f].n_lines) {
                    const uint64_t b = line_begin(runs[f], (uint64_t)runs[f].skip_lines + files[f].first + res.P);
                    cursor[f] = b < runs[f].len ? b : runs[f].len;
                }
        std::fprintf(out, "%u %u %u %u %u %u", res.P, res.done, res.err, res.err_file, res.err_line, res.err_file2);
        for (unsigned f = 0; f < F; ++f)
            std::fprintf(out, " %u %u %u %u %llu", files[f].n_lines, files[f].first, files[f].n_in, files[f].term, (unsigned long long)cursor[f]);
        std::fprintf(out, "\n");
        ++n_cases;
        int c = std::fgetc(in);
        if (c != EOF) std::ungetc(c, in);
    }
    if (!std::feof(in)) die("trailing bytes that are no CASE");
    std::fclose(in);
    if (std::fclose(out) != 0) die("cannot write the answers");
    std::printf("text_region_check: %zu cases, tile %llu\n", n_cases, (unsigned long long)tile_bytes);
    return 0;
}
