// Test harness (tests/ only): the definition of the rows of a SAMPLE PART, bv_ptext_row_part of
// basevar_amd/csrc/bv_pileup_text_core.h, against the host's writer: the rows of part [s0, s1) are, byte for byte, what
// pileup_rows_text() of basevar_amd/host/pileup.hpp writes for a PileupTile sliced to the part's columns, with the samples of
// its indel tokens rebased.  A program of its own (tests/test_pileup_text_parts_cpu.py builds it with ASan + UBSan and runs it);
// it links nothing of the engine.
//   pileup_text_parts_check random
//       the seeded value-range tiles of pileup_text_check.cpp's kind (n 1 .. 75, every plane over its whole range, tokens to 200
//       bytes), each under several seeded part tables: parts of one sample, all samples as one part, gaps before and behind.
//   pileup_text_parts_check tile <tile.bin> <text.out> <first sample of part 0> <of part 1> ... <end of the last part>
//       one tile from a file (tests/pileup_text_model.py writes it): the parts' text of its rows [first, first + n_rows), part-major,
//       goes to text.out with its row offsets -- what the GPU tests expect of the device --, after every part was held to the host
//       writer.  An indel cell without a token inside a part ends the run with status 1 in text.out, its pos and ABSOLUTE sample
//       beside it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "../../basevar_amd/csrc/bv_pileup_text_core.h"
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

// the tile that holds only columns [s0, s1) of t: planes copied, depths counted, tokens of those columns with samples rebased
PileupTile slice(const PileupTile &t, uint32_t s0, uint32_t s1) {
    PileupTile p;
    p.reset(t.ref_id, t.beg, t.end, s1 - s0);
    for (size_t r = 0; r < t.rows(); ++r)
        for (uint32_t s = s0; s < s1; ++s) {
            const size_t from = r * t.pitch + s, to = r * p.pitch + (s - s0);
            p.cell[to] = t.cell[from]; p.qual[to] = t.qual[from]; p.mapq[to] = t.mapq[from]; p.rank[to] = t.rank[from];
        }
    p.depth.assign(p.rows(), 0);
    for (size_t r = 0; r < p.rows(); ++r)
        for (size_t s = 0; s < p.n_samples; ++s) p.depth[r] += p.rank[r * p.pitch + s] != 0;
    for (const auto &i : t.indels)
        if (i.sample >= s0 && i.sample < s1) p.indels.push_back({i.pos, i.sample - s0, i.text});
    return p;
}

// the core over rows [first, first + n_rows) of part [s0, s1); false where a cell of the part has no token
bool core_part(const PileupTile &t, const Tokens &k, const std::string &fa, uint32_t s0, uint32_t s1, uint32_t first, uint32_t n_rows, std::string &out,
               std::vector<uint64_t> &off, uint32_t *bad_pos, uint32_t *bad_sample) {
    for (uint32_t r = first; r < first + n_rows; ++r) {
        const size_t at = (size_t)r * t.pitch;
        const uint32_t pos = t.beg + r;
        const uint8_t *text = reinterpret_cast<const uint8_t *>(k.text.data());
        const uint64_t len = bv_ptext_row_part(t.ref_id.data(), (uint32_t)t.ref_id.size(), pos, (uint8_t)fa[pos - 1], &t.cell[at], &t.qual[at], &t.mapq[at], &t.rank[at],
                                               s0, s1, k.tok.data(), k.tok.size(), text, nullptr, bad_sample);
        if (len == 0) { *bad_pos = pos; return false; }
        const size_t o = out.size();
        out.resize(o + len);
        const uint64_t put = bv_ptext_row_part(t.ref_id.data(), (uint32_t)t.ref_id.size(), pos, (uint8_t)fa[pos - 1], &t.cell[at], &t.qual[at], &t.mapq[at], &t.rank[at],
                                               s0, s1, k.tok.data(), k.tok.size(), text, reinterpret_cast<uint8_t *>(&out[o]), bad_sample);
        if (put != len) { std::cerr << "the count and the write of a row differ\n"; std::exit(1); }
        off.push_back(out.size());
    }
    return true;
}

int fail_at(const std::string &what, const std::string &got, const std::string &exp) {
    size_t at = 0;
    while (at < got.size() && at < exp.size() && got[at] == exp[at]) ++at;
    std::cerr << what << ": texts differ at byte " << at << " (" << got.size() << " / " << exp.size() << " bytes)\n  core: "
              << got.substr(at > 40 ? at - 40 : 0, 120) << "\n  host: " << exp.substr(at > 40 ? at - 40 : 0, 120) << "\n";
    return 1;
}

// every part of the table against the host writer on the sliced tile; the whole rows, and rows [first, first + n_rows) as a slice
// of them.  0, 1 (differs) or 3 (a token is missing in a part)
int check_parts(const PileupTile &t, const Tokens &k, const std::string &fa, const std::vector<uint32_t> &part_first, uint32_t first, uint32_t n_rows,
                const std::string &what) {
    for (size_t p = 0; p + 1 < part_first.size(); ++p) {
        const uint32_t s0 = part_first[p], s1 = part_first[p + 1];
        std::string core, host, sub;
        std::vector<uint64_t> off(1, 0), sub_off(1, 0);
        uint32_t bp = 0, bs = 0;
        if (!core_part(t, k, fa, s0, s1, 0, (uint32_t)t.rows(), core, off, &bp, &bs)) return 3;
        pileup_rows_text(slice(t, s0, s1), fa, host);
        if (core != host) return fail_at(what + " part " + std::to_string(p), core, host);
        if (!core_part(t, k, fa, s0, s1, first, n_rows, sub, sub_off, &bp, &bs)) return 3;
        if (sub != host.substr(off[first], off[first + n_rows] - off[first])) return fail_at(what + " sub-range of part " + std::to_string(p), sub, host);
    }
    return 0;
}

int run_random() {
    uint64_t st = 0x2545f4914f6cdd1dull;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    size_t n_rows = 0, n_parts = 0, n_indels = 0, longest = 0, n_gaps = 0, n_single = 0;
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
            }
        const Tokens k = tokens_of(t);
        // part tables: all samples as one part; parts of one sample; seeded cuts with gaps before and behind
        std::vector<std::vector<uint32_t>> tables;
        tables.push_back({0, (uint32_t)n});
        {
            std::vector<uint32_t> ones;
            for (uint32_t s = 0; s <= n; ++s) ones.push_back(s);
            tables.push_back(ones);
        }
        for (int j = 0; j < 3; ++j) {
            std::vector<uint32_t> cuts;
            uint32_t at = (uint32_t)(rnd() % (n + 1) / 3);
            while (at < n && cuts.size() < 9) {
                cuts.push_back(at);
                at += 1 + (uint32_t)(rnd() % (1 + n / 2));
            }
            cuts.push_back(std::min<uint32_t>(at, (uint32_t)n));
            if (cuts.size() < 2 || cuts[cuts.size() - 2] >= cuts.back()) continue;
            n_gaps += cuts.front() > 0 || cuts.back() < n;
            tables.push_back(cuts);
        }
        for (const auto &table : tables) {
            const uint32_t first = (uint32_t)(rnd() % len), cnt = (uint32_t)(rnd() % (len - first + 1));
            const int rc = check_parts(t, k, fa, table, first, cnt, "round " + std::to_string(round));
            if (rc) { std::cerr << "round " << round << ": status " << rc << "\n"; return 1; }
            n_parts += table.size() - 1;
            n_single += table.size() - 1 == n;
        }
        n_rows += len;
    }
    std::cout << "PILEUP_TEXT_PARTS rounds 80 rows " << n_rows << " parts " << n_parts << " tables with gaps " << n_gaps << " indel tokens " << n_indels << " longest "
              << longest << " FAILS 0" << std::endl;
    return longest >= 150 && n_indels > 1000 && n_gaps > 20 && n_single >= 80 ? 0 : 1;
}

template <typename T>
void get(FILE *f, T *p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) { std::cerr << "tile file too short\n"; std::exit(2); }
}

int run_tile(int argc, char **argv) {
    const char *path = argv[2], *out_path = argv[3];
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
    std::vector<uint32_t> part_first;
    for (int i = 4; i < argc; ++i) part_first.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
    for (size_t p = 0; p + 1 < part_first.size(); ++p)
        if (part_first[p] >= part_first[p + 1]) { std::cerr << "parts must ascend\n"; return 2; }
    if (part_first.size() < 2 || part_first.back() > h[2]) { std::cerr << "bad parts\n"; return 2; }
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
    Tokens k;
    k.tok = tok; k.text = text;
    // the asked-for rows, part-major; they alone decide the status the device has to give
    std::string out;
    std::vector<uint64_t> off(1, 0);
    uint32_t bad_pos = 0, bad_sample = 0, status = 0;
    for (size_t p = 0; p + 1 < part_first.size() && !status; ++p)
        if (!core_part(t, k, fa, part_first[p], part_first[p + 1], h[6], h[7], out, off, &bad_pos, &bad_sample)) status = 1;
    bool held = false;
    if (!status) {
        const int rc = check_parts(t, k, fa, part_first, h[6], h[7], "tile");
        if (rc == 1) return 1;
        held = rc == 0;  // (3: a row outside the asked-for ones misses a token: the host writer has no answer for the whole tile)
    }
    FILE *o = std::fopen(out_path, "wb");
    if (!o) { std::cerr << "cannot write " << out_path << "\n"; return 2; }
    const uint32_t n_out = status ? 0 : (uint32_t)(off.size() - 1);
    const uint32_t head[4] = {status, n_out, bad_pos, bad_sample};
    std::fwrite("PTXT", 1, 4, o);
    std::fwrite(head, 4, 4, o);
    if (!status) {
        std::fwrite(off.data(), 8, off.size(), o);
        std::fwrite(out.data(), 1, out.size(), o);
    }
    std::fclose(o);
    std::cout << "status " << status << " parts " << part_first.size() - 1 << " rows " << h[7] << " bytes " << out.size() << (held ? " host == core" : " (core only)") << std::endl;
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "random")) return run_random();
    if (argc >= 6 && !std::strcmp(argv[1], "tile")) return run_tile(argc, argv);
    std::cerr << "usage: pileup_text_parts_check random | tile <tile.bin> <text.out> <part_first ...>\n";
    return 2;
}
