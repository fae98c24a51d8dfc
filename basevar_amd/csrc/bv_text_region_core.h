// bv_text_region_core.h -- the rows of a region (include/basevar_amd_region.h): which lines of every batchfile's inflated run a
// call of bv_engine_text_parse_bgzf_region takes, stated on bytes and without reference to lanes.  The kernels of bv_text.hip
// compile these functions and are their schedule; tests/cpp/text_region_check.cpp compiles them with g++ and holds them to a
// serial model that shares no code with them (tests/text_region_model.py).
//
// THE DEFINITION.  A region is (name bytes, beg, end), 1-based inclusive, beg <= end.  Per file, the LINES are the complete
// lines behind skip_bytes and then skip_lines, exactly as the line index counts them (with at_end, a last line without a line
// break is a line); a line's ORDINAL is its index among them, from 0.  The HEAD of a line: CHROM = the bytes before its first
// tab; POS = the 1 to 10 decimal digits between its first and second tab, value <= 2^32 - 1.  A line without two tabs, or
// whose POS is anything else, has a MALFORMED head.  A line is REACHED when CHROM == name and POS >= beg; it is IN when it is
// also <= end.  (A malformed line is neither.)
//   first[f] = the ordinal of file f's first reached line; n_in[f] = the number of consecutive IN lines from there.  The
//   selection ends at the first line at or behind first[f] that is not IN: the file's TERMINATING line.  A run without a
//   reached line: first[f] = the number of its lines (all of them count as skipped), n_in[f] = 0, no terminating line.
//   P = min(max_positions, cfg.max_sites, min over f of n_in[f]); row (p, f) is line first[f] + p.
//   cursor[f] = the start of line first[f] + P: skipped lines are consumed, so a call always makes progress.  A file without a
//   line is left where it was (its skip_lines are still to be skipped).
//   A file has TERMINATED when n_in[f] == P and (it has a terminating line, or at_end).  region_done = every file has.
// Refusals (BV_ERR_DATA), in this order:
//   BV_TR_ERR_HEAD   a malformed head at or before a file's terminating line (anywhere in the run, where it has none); the
//                    lowest such file and its lowest such line.  Behind the terminating line heads are not looked at.
//   BV_TR_ERR_COUNT  P < min(max_positions, cfg.max_sites), a file has terminated and another has IN lines beyond P: the
//                    lowest terminated file and the lowest file with more.
//   BV_TR_ERR_POS    POS of row (p, f) != POS of row (p, 0): the lowest such p, then f.
// This is what a tabix query returns on files sorted by position, the only kind an index can be built of.
//
// THE WALK.  A run is cut into tiles and a tile is walked in steps of 64 bytes.  The line that begins behind a line break
// belongs to the step (and tile) of the line break; the run's first line belongs to a step of its own in front of the first
// tile.  Of a step only four 64-bit masks are looked at (bit k = byte k of the step):
//   LS   the byte is a line break and the line behind it has an ordinal (it is not one of the skip_lines)
//   RE, NI, MA   ... and that line is reached; is not IN; is malformed (MA is a part of NI)
// with q0, the ordinal of the line of LS's lowest bit.  bv_tr_step() folds a step into its tile's summary (bv_tr_tile),
// bv_tr_file_add() folds the tiles of a file in order, bv_tr_file_finish() gives the file's first / n_in / terminating line,
// and bv_tr_decide() gives P, region_done and the refusal.  The line behind the run's LAST line break is no line (it has no
// line break of its own) but is folded like one: its ordinal is the number of lines, larger than any real one, so
// bv_tr_file_finish() drops whatever it left by comparing with that number.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BV_TR_FN __host__ __device__ __forceinline__
#else
#define BV_TR_FN inline
#endif

#define BV_TR_NONE 0xFFFFFFFFu
#define BV_TR_MAL 1u      // bv_tr_head: the head is malformed
#define BV_TR_REACHED 2u  //             CHROM == name and POS >= beg
#define BV_TR_IN 4u       //             ... and POS <= end
#define BV_TR_ERR_HEAD 1u
#define BV_TR_ERR_COUNT 2u
#define BV_TR_ERR_POS 3u

struct bv_tr_region {
    const char *name;
    uint32_t name_len, beg, end;
};

// The head of the line p[0 .. n): n = the bytes from the line's first byte to the end of the run (the line break, where the
// line has one, is among them; the walk stops there).  *pos = POS where the head is well-formed.
BV_TR_FN uint32_t bv_tr_head(const char *p, uint64_t n, const bv_tr_region &rg, uint32_t *pos) {
    uint64_t i = 0;
    bool same = true;
    for (; i < n && p[i] != '\t' && p[i] != '\n'; ++i) same = same && i < rg.name_len && p[i] == rg.name[i];
    if (i >= n || p[i] != '\t') return BV_TR_MAL;
    same = same && i == rg.name_len;
    uint64_t v = 0;
    uint32_t digits = 0;
    for (++i; i < n && p[i] >= '0' && p[i] <= '9'; ++i) {
        if (++digits > 10u) return BV_TR_MAL;
        v = v * 10u + (uint64_t)(p[i] - '0');
    }
    if (i >= n || p[i] != '\t' || digits == 0 || v > 0xFFFFFFFFull) return BV_TR_MAL;
    *pos = (uint32_t)v;
    if (!same || v < rg.beg) return 0u;
    return v <= rg.end ? (BV_TR_REACHED | BV_TR_IN) : BV_TR_REACHED;
}

BV_TR_FN uint32_t bv_tr_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}
BV_TR_FN uint32_t bv_tr_low(uint64_t x) {  // index of the lowest set bit, x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__ffsll((long long)x) - 1u;
#else
    return (uint32_t)__builtin_ctzll(x);
#endif
}
BV_TR_FN uint64_t bv_tr_below(uint32_t k) { return (1ull << k) - 1ull; }  // k < 64

// What a tile's lines leave: ordinals, BV_TR_NONE where there is no such line.
struct bv_tr_tile {
    uint32_t cnt;  // line breaks in the tile
    uint32_t r;    // the lowest reached line
    uint32_t nb;   // the lowest line at or behind r that is not IN
    uint32_t a;    // the lowest line that is not IN
    uint32_t m;    // the lowest malformed line
    uint32_t reserved_[3];
};

BV_TR_FN bv_tr_tile bv_tr_tile_init() {
    bv_tr_tile t;
    t.cnt = 0; t.r = t.nb = t.a = t.m = BV_TR_NONE;
    t.reserved_[0] = t.reserved_[1] = t.reserved_[2] = 0;
    return t;
}

// ordinal of the line of LS's bit k
BV_TR_FN uint32_t bv_tr_ordinal_at(uint64_t LS, uint32_t q0, uint32_t k) { return q0 + bv_tr_popc(LS & bv_tr_below(k)); }

BV_TR_FN void bv_tr_step(bv_tr_tile &t, uint64_t LS, uint64_t RE, uint64_t NI, uint64_t MA, uint32_t q0) {
    if (!LS) return;
    if (t.r == BV_TR_NONE) {
        if (RE) {
            const uint32_t k = bv_tr_low(RE);
            t.r = bv_tr_ordinal_at(LS, q0, k);
            const uint64_t behind = NI & ~bv_tr_below(k);  // (the reached line itself, where it lies beyond `end`)
            if (behind) t.nb = bv_tr_ordinal_at(LS, q0, bv_tr_low(behind));
        }
    } else if (t.nb == BV_TR_NONE && NI) {
        t.nb = bv_tr_ordinal_at(LS, q0, bv_tr_low(NI));
    }
    if (t.a == BV_TR_NONE && NI) t.a = bv_tr_ordinal_at(LS, q0, bv_tr_low(NI));
    if (t.m == BV_TR_NONE && MA) t.m = bv_tr_ordinal_at(LS, q0, bv_tr_low(MA));
}

// What a file's run says.
struct bv_tr_file {
    uint32_t n_lines;  // its lines
    uint32_t first;    // the first reached line; n_lines where there is none
    uint32_t n_in;     // IN lines from there
    uint32_t term;     // 1: a terminating line lies in the run (line first + n_in)
    uint32_t mal;      // the malformed line that refuses the run, or BV_TR_NONE
    uint32_t r, e, m;  // while the tiles are folded: the lowest reached line, the terminating line, the lowest malformed line
};

BV_TR_FN bv_tr_file bv_tr_file_init() {
    bv_tr_file f;
    f.n_lines = f.first = f.n_in = f.term = 0;
    f.mal = f.r = f.e = f.m = BV_TR_NONE;
    return f;
}

// the tiles of a file, in order
BV_TR_FN void bv_tr_file_add(bv_tr_file &f, const bv_tr_tile &t) {
    if (f.m == BV_TR_NONE) f.m = t.m;
    if (f.r == BV_TR_NONE) {
        if (t.r != BV_TR_NONE) { f.r = t.r; f.e = t.nb; }
    } else if (f.e == BV_TR_NONE) {
        f.e = t.a;
    }
}

// n_breaks: the line breaks of the run behind skip_bytes (the spare one of an unterminated last line with at_end among them)
BV_TR_FN void bv_tr_file_finish(bv_tr_file &f, uint32_t n_breaks, uint32_t skip_lines) {
    const uint32_t n = n_breaks > skip_lines ? n_breaks - skip_lines : 0u;
    if (f.r != BV_TR_NONE && f.r >= n) f.r = f.e = BV_TR_NONE;
    if (f.e != BV_TR_NONE && f.e >= n) f.e = BV_TR_NONE;
    if (f.m != BV_TR_NONE && f.m >= n) f.m = BV_TR_NONE;
    f.n_lines = n;
    f.first = f.r == BV_TR_NONE ? n : f.r;
    f.n_in = f.r == BV_TR_NONE ? 0u : (f.e == BV_TR_NONE ? n : f.e) - f.r;
    f.term = f.e != BV_TR_NONE ? 1u : 0u;
    f.mal = (f.m != BV_TR_NONE && (f.e == BV_TR_NONE || f.m <= f.e)) ? f.m : BV_TR_NONE;
}

struct bv_tr_result {
    uint32_t P, done;
    uint32_t err;       // 0, or BV_TR_ERR_*
    uint32_t err_file;  // HEAD: the file; COUNT: the terminated file; POS: the file that differs from file 0
    uint32_t err_line;  // HEAD: the line's ordinal; COUNT: the terminated file's line first + P; POS: the position p
    uint32_t err_file2; // COUNT: the file with IN lines beyond P
    uint32_t reserved_[2];
};

BV_TR_FN bool bv_tr_terminated(const bv_tr_file &f, uint32_t P, uint32_t at_end) { return f.n_in == P && (f.term || at_end); }

// P, region_done and the first two refusals, from the files' results; cap = min(max_positions, cfg.max_sites)
BV_TR_FN bv_tr_result bv_tr_decide(const bv_tr_file *f, uint32_t F, uint32_t cap, uint32_t at_end) {
    bv_tr_result r;
    r.P = cap; r.done = 1; r.err = 0; r.err_file = r.err_line = r.err_file2 = 0; r.reserved_[0] = r.reserved_[1] = 0;
    for (uint32_t k = 0; k < F; ++k) r.P = f[k].n_in < r.P ? f[k].n_in : r.P;
    uint32_t ended = BV_TR_NONE, more = BV_TR_NONE;
    for (uint32_t k = 0; k < F; ++k) {
        if (f[k].mal != BV_TR_NONE && !r.err) { r.err = BV_TR_ERR_HEAD; r.err_file = k; r.err_line = f[k].mal; }
        const bool t = bv_tr_terminated(f[k], r.P, at_end);
        if (!t) r.done = 0;
        if (t && ended == BV_TR_NONE) ended = k;
        if (f[k].n_in > r.P && more == BV_TR_NONE) more = k;
    }
    if (!r.err && r.P < cap && ended != BV_TR_NONE && more != BV_TR_NONE) {
        r.err = BV_TR_ERR_COUNT; r.err_file = ended; r.err_line = f[ended].first + r.P; r.err_file2 = more;
    }
    if (r.err) { r.P = 0; r.done = 0; }
    return r;
}
