// Test harness (tests/ only): the device row writer's definition, basevar_amd/csrc/bv_pileup_text_core.h, against the host's
// writer, pileup_rows_text() of basevar_amd/host/pileup.hpp, byte for byte.  A program of its own (tests/test_pileup_text_cpu.py
// builds it with ASan + UBSan and runs it); it links nothing of the engine.
//   pileup_text_check random
//       seeded random tiles with the value range of pileup_rows_check.cpp and beyond it: n 1 .. 75, mapq 0-255, quals 0-255, ranks
//       to 65,535, N calls, insertions, deletions (tokens to 200 bytes), both strands, uncovered rows, reference letters
//       ACGTNacgt; the whole tile's text and sub-ranges of it.
//   pileup_text_check tile <tile.bin> <text.out>
//       one tile from a file (tests/pileup_text_model.py writes it): the core's text of its rows [first, first + n_rows) goes to
//       text.out with its row offsets -- what the GPU tests expect of the device --, after the whole tile's text was held to the
//       host writer's.  An indel cell without a token ends the run with status 1 in text.out: the host writer has no answer there.
//   pileup_text_check time <n_samples> <rows> <coverage percent> [level]
//       timing only (built without sanitizers): the text by pileup_rows_text, and BgzfWriter over it, on this thread.
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "../../basevar_amd/csrc/bv_pileup_text_core.h"
#include "../../basevar_amd/host/bgzf_tabix.hpp"
#include "../../basevar_amd/host/pileup.hpp"

using namespace bvamd;

namespace {

struct Tokens {
    std::vector<BvPtextToken> tok;
    std::string text;
};

Tokens tokens_of(const PileupTile &t) {
    Tokens k;
    for (const auto &i : t.indels) {
        k.tok.push_back({i.pos, i.sample, (uint64_t)k.text.size(), (uint32_t)i.text.size(), 0});
        k.text += i.text;
    }
    return k;
}

// the core over rows [first, first + n_rows) of the tile; false where a cell has no token
bool core_text(const PileupTile &t, const Tokens &k, const std::string &fa, uint32_t first, uint32_t n_rows, std::string &out, std::vector<uint64_t> &off,
               uint32_t *bad_pos, uint32_t *bad_sample) {
    out.clear();
    off.assign(1, 0);
    const uint32_t n = (uint32_t)t.n_samples;
    for (uint32_t r = first; r < first + n_rows; ++r) {
        const size_t at = (size_t)r * t.pitch;
        const uint32_t pos = t.beg + r;
        const uint8_t *text = reinterpret_cast<const uint8_t *>(k.text.data());
        const uint64_t len = bv_ptext_row(t.ref_id.data(), (uint32_t)t.ref_id.size(), pos, (uint8_t)fa[pos - 1], &t.cell[at], &t.qual[at], &t.mapq[at], &t.rank[at], n,
                                          k.tok.data(), k.tok.size(), text, nullptr, bad_sample);
        if (len == 0) { *bad_pos = pos; return false; }
        const size_t o = out.size();
        out.resize(o + len);
        const uint64_t put = bv_ptext_row(t.ref_id.data(), (uint32_t)t.ref_id.size(), pos, (uint8_t)fa[pos - 1], &t.cell[at], &t.qual[at], &t.mapq[at], &t.rank[at], n,
                                          k.tok.data(), k.tok.size(), text, reinterpret_cast<uint8_t *>(&out[o]), bad_sample);
        if (put != len) { std::cerr << "the count and the write of a row differ\n"; std::exit(1); }
        off.push_back(out.size());
    }
    return true;
}

void fill_depth(PileupTile &t) {
    t.depth.assign(t.rows(), 0);
    for (size_t r = 0; r < t.rows(); ++r)
        for (size_t s = 0; s < t.n_samples; ++s) t.depth[r] += t.rank[r * t.pitch + s] != 0;
}

int fail_at(const char *what, const std::string &got, const std::string &exp) {
    size_t at = 0;
    while (at < got.size() && at < exp.size() && got[at] == exp[at]) ++at;
    std::cerr << what << ": texts differ at byte " << at << " (" << got.size() << " / " << exp.size() << " bytes)\n  core: "
              << got.substr(at > 40 ? at - 40 : 0, 120) << "\n  host: " << exp.substr(at > 40 ? at - 40 : 0, 120) << "\n";
    return 1;
}

int run_random() {
    uint64_t st = 0x2545f4914f6cdd1dull;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    size_t n_rows = 0, n_cells = 0, n_indels = 0, n_sub = 0, longest = 0;
    for (int round = 0; round < 80; ++round) {
        const size_t n = 1 + rnd() % 75;
        const uint32_t beg = round % 9 == 0 ? 99990 + (uint32_t)(rnd() % 10) : 1 + (uint32_t)(rnd() % 500), len = 1 + (uint32_t)(rnd() % 40), end = beg + len - 1;
        std::string fa(end + 5, 'A');
        for (char &c : fa) c = "ACGTNacgt"[rnd() % 9];
        PileupTile t;
        t.reset("chr" + std::to_string(1 + round % 22), beg, end, n);
        const int cover = round % 7 == 0 ? 0 : round % 7 == 1 ? 100 : (int)(rnd() % 100);
        for (uint32_t pos = beg; pos <= end; ++pos)
            for (size_t i = 0; i < n; ++i) {
                const size_t k = t.at(pos, i);
                if ((int)(rnd() % 100) >= cover) {  // unclaimed: the other planes may hold anything
                    if (rnd() & 1) { t.cell[k] = (uint8_t)(rnd() % 16); t.qual[k] = (uint8_t)rnd(); t.mapq[k] = (uint8_t)rnd(); }
                    continue;
                }
                const bool rev = rnd() & 1;
                const int kind = (int)(rnd() % 12);
                const char b = "ACGT"[rnd() & 3];
                t.mapq[k] = (uint8_t)(rnd() % 256);
                t.qual[k] = (uint8_t)(rnd() % 256);
                t.rank[k] = (uint16_t)(1 + rnd() % (rnd() % 8 ? 150 : 65535));
                if (kind == 0) t.cell[k] = (uint8_t)(BV_CELL_N | (rev ? BV_CELL_REV : 0));
                else if (kind <= 2) {
                    std::string s;
                    for (int j = 0, m = 1 + (int)(rnd() % (rnd() % 10 ? 4 : 198)); j < m; ++j) s += "ACGTacgt"[rnd() & 7];
                    t.cell[k] = (uint8_t)((kind == 1 ? BV_CELL_INS : BV_CELL_DEL) | (rev ? BV_CELL_REV : 0));
                    t.indels.push_back({pos, (uint32_t)i, std::string(kind == 1 ? "+" : "-") + b + s});
                    longest = std::max(longest, t.indels.back().text.size());
                    ++n_indels;
                } else t.cell[k] = (uint8_t)(pileup_base_code(b) | (rev ? BV_CELL_REV : 0));
                ++n_cells;
            }
        fill_depth(t);
        std::string host, core, part;
        std::vector<uint64_t> off, part_off;
        uint32_t bp = 0, bs = 0;
        pileup_rows_text(t, fa, host);
        const Tokens k = tokens_of(t);
        if (!core_text(t, k, fa, 0, len, core, off, &bp, &bs)) { std::cerr << "round " << round << ": a token is missing\n"; return 1; }
        if (core != host) return fail_at(("round " + std::to_string(round)).c_str(), core, host);
        for (int j = 0; j < 4; ++j) {  // sub-ranges: single rows, the last row, the empty range
            const uint32_t first = j == 0 ? len - 1 : (uint32_t)(rnd() % len), cnt = j == 0 ? 1 : j == 1 ? 0 : 1 + (uint32_t)(rnd() % (len - first));
            if (!core_text(t, k, fa, first, cnt, part, part_off, &bp, &bs)) return 1;
            if (part != host.substr(off[first], off[first + cnt] - off[first])) return fail_at("sub-range", part, host.substr(off[first], off[first + cnt] - off[first]));
            ++n_sub;
        }
        n_rows += len;
    }
    std::cout << "PILEUP_TEXT rounds 80 rows " << n_rows << " claimed cells " << n_cells << " indel tokens " << n_indels << " longest " << longest << " sub-ranges "
              << n_sub << " FAILS 0" << std::endl;
    return longest >= 150 && n_indels > 1000 ? 0 : 1;
}

template <typename T>
void get(FILE *f, T *p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) { std::cerr << "tile file too short\n"; std::exit(2); }
}

int run_tile(const char *path, const char *out_path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::cerr << "cannot open " << path << "\n"; return 2; }
    char magic[4];
    uint32_t h[8];
    uint64_t w[2];
    get(f, magic, 4);
    get(f, h, 8);  // beg, rows, n, pitch, n_tokens, chrom_len, first, n_rows
    get(f, w, 2);  // text_bytes, ref_len
    if (std::memcmp(magic, "PTIL", 4) != 0 || h[1] == 0 || h[2] == 0 || h[3] < h[2] || (uint64_t)h[6] + h[7] > h[1] || (uint64_t)h[0] + h[1] - 1 > w[1] || h[0] == 0) {
        std::cerr << "bad tile file\n";
        return 2;
    }
    PileupTile t;
    std::string fa(w[1], 'A'), text(w[0], '\0');
    t.ref_id.assign(h[5], '\0');
    t.beg = h[0]; t.end = h[0] + h[1] - 1; t.n_samples = h[2]; t.pitch = h[3];
    const size_t cells = (size_t)h[1] * h[3];
    t.cell.resize(cells); t.qual.resize(cells); t.mapq.resize(cells); t.rank.resize(cells);
    std::vector<BvPtextToken> tok(h[4]);
    get(f, &t.ref_id[0], h[5]); get(f, &fa[0], w[1]);
    get(f, t.cell.data(), cells); get(f, t.qual.data(), cells); get(f, t.mapq.data(), cells); get(f, t.rank.data(), cells);
    get(f, tok.data(), tok.size()); get(f, &text[0], w[0]);
    std::fclose(f);
    for (size_t k = 0; k < tok.size(); ++k) {
        if (tok[k].text_off > w[0] || tok[k].text_len > w[0] - tok[k].text_off) { std::cerr << "token text out of bounds\n"; return 2; }
        if (k && !(tok[k - 1].pos < tok[k].pos || (tok[k - 1].pos == tok[k].pos && tok[k - 1].sample < tok[k].sample))) { std::cerr << "tokens out of order\n"; return 2; }
        t.indels.push_back({tok[k].pos, tok[k].sample, text.substr(tok[k].text_off, tok[k].text_len)});
    }
    fill_depth(t);
    Tokens k;
    k.tok = tok; k.text = text;
    std::string core, host, part;
    std::vector<uint64_t> off, part_off;
    uint32_t bad_pos = 0, bad_sample = 0, status = 0;
    if (!core_text(t, k, fa, 0, h[1], core, off, &bad_pos, &bad_sample)) {
        status = 1;
        // (only the asked-for rows decide the status the device has to give)
        if (core_text(t, k, fa, h[6], h[7], part, part_off, &bad_pos, &bad_sample)) status = 0;
    } else {
        pileup_rows_text(t, fa, host);
        if (core != host) return fail_at("tile", core, host);
        if (!core_text(t, k, fa, h[6], h[7], part, part_off, &bad_pos, &bad_sample)) return 1;
        if (part != host.substr(off[h[6]], off[h[6] + h[7]] - off[h[6]])) return fail_at("sub-range", part, host);
    }
    FILE *o = std::fopen(out_path, "wb");
    if (!o) { std::cerr << "cannot write " << out_path << "\n"; return 2; }
    const uint32_t head[4] = {status, status ? 0 : h[7], bad_pos, bad_sample};
    std::fwrite("PTXT", 1, 4, o);
    std::fwrite(head, 4, 4, o);
    if (!status) {
        std::fwrite(part_off.data(), 8, part_off.size(), o);
        std::fwrite(part.data(), 1, part.size(), o);
    }
    std::fclose(o);
    std::cout << "status " << status << " rows " << h[7] << " bytes " << part.size() << (host.empty() ? " (core only)" : " host == core") << std::endl;
    return 0;
}

int run_time(int argc, char **argv) {
    const size_t n = std::strtoull(argv[2], nullptr, 10);
    const uint32_t rows = (uint32_t)std::strtoul(argv[3], nullptr, 10), cover = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    const int level = argc > 5 ? std::atoi(argv[5]) : 6;
    uint64_t st = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    PileupTile t;
    t.reset("chr1", 1, rows, n);
    std::string fa(rows + 1, 'A');
    for (uint32_t pos = 1; pos <= rows; ++pos)
        for (size_t i = 0; i < n; ++i) {
            if (rnd() % 100 >= cover) continue;
            const size_t k = t.at(pos, i);
            t.cell[k] = (uint8_t)(rnd() & 7); t.qual[k] = (uint8_t)(rnd() % 42); t.mapq[k] = (uint8_t)(rnd() % 61); t.rank[k] = (uint16_t)(1 + rnd() % 150);
        }
    fill_depth(t);
    std::string text;
    const auto t0 = std::chrono::steady_clock::now();
    pileup_rows_text(t, fa, text);
    const auto t1 = std::chrono::steady_clock::now();
    const std::string out = "/tmp/pileup_text_check." + std::to_string((long)getpid()) + ".gz";
    {
        BgzfWriter wtr;
        wtr.open(out, level);
        wtr.write(text.data(), text.size());
        wtr.close();
    }
    const auto t2 = std::chrono::steady_clock::now();
    std::remove(out.c_str());
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::cout << "TIME samples " << n << " rows " << rows << " coverage " << cover << " text_bytes " << text.size() << " rows_text_ms " << ms(t0, t1)
              << " bgzf_level " << level << " bgzf_ms " << ms(t1, t2) << std::endl;
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "random")) return run_random();
    if (argc == 4 && !std::strcmp(argv[1], "tile")) return run_tile(argv[2], argv[3]);
    if (argc >= 5 && !std::strcmp(argv[1], "time")) return run_time(argc, argv);
    std::cerr << "usage: pileup_text_check random | tile <tile.bin> <text.out> | time <n_samples> <rows> <coverage percent> [level]\n";
    return 2;
}
