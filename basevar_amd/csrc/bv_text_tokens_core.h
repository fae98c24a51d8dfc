// bv_text_tokens_core.h -- the indel tokens of parsed batchfile rows (include/basevar_amd_text_tokens.h): which bytes of a
// batch's rows are '+SEQ' / '-SEQ' tokens of the Readbases column, stated on bytes and without reference to lanes.  The kernels
// of bv_text_tokens.hip compile these functions and are their schedule; tests/cpp/text_tokens_check.cpp compiles them with g++
// and holds them to the tokens that the host reader and BaseTypeEngine::finish_text's walk collect, byte for byte.
//
// THE DEFINITION.  A parsed batch has P positions x F files; row (p, f) is the bytes of file f's line of position p, the last
// of them '\n'.  A row's fields are separated by tabs, field 5 (counting from 0) is Readbases, and a field's tokens are
// separated by single spaces.  The token list holds every token that
//   * is a token of field 5 of a row of a position whose FINAL row_state is 0 (not BV_TEXT_SKIP, not BV_TEXT_HOST: positions
//     the parse refused are BV_TEXT_HOST),
//   * whose first byte is '+' or '-';
//   its text is the bytes up to the next space or tab (at least the sign: a bare '+' is a token; no upper bound).
// Order: position ascending, then file ascending, then the token's place in its column.  A token's descriptor has pos = the
// position's INDEX in the batch (0 .. P-1, not the genomic POS), sample = foff[f] + the token's index in its column, text_len
// its byte count, and text_off ascending and non-overlapping in one text buffer.  No other field's '+' / '-' is a token: not
// the Strand column's, not a quality of '+' (phred 10) or '-' (phred 12), not a '-' inside CHROM or REF.
//
// THE WALK.  A row is walked in steps of 64 bytes.  Of a step only six 64-bit masks are looked at (bit k = byte k of the step):
//   T, S, SEP   the byte is a tab; a space; a tab, space or line break
//   V           the byte lies inside the row
//   F5          the byte lies in field 5: the tabs before it in the row number 5
//   PM          the byte is '+' or '-'
// and four numbers carried from step to step (bv_tt_carry): the field and the column's token index at the step's first byte,
// whether the byte before the step was a separator, and whether it was a byte of an indel token (`open`: such a token may
// span any number of steps).  bv_tt_step_masks() gives the step's
//   M    bytes that are text of an indel token,
//   IS   first bytes of indel tokens that begin in the step,
//   EN   separators that end an indel token,
// and the bv_tt_*_at(k) functions give what the byte at k writes: its place in the text, its token's ordinal in the row, and
// for an ending separator the token's length -- from the step's masks where the token began in the step, from the carry where
// it did not.  A count pass keeps only n_tok and n_txt; a write pass that goes through the same functions cannot disagree.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BV_TT_FN __host__ __device__ __forceinline__
#else
#define BV_TT_FN inline
#endif

#define BV_TT_FIELD 5u  // Readbases

// one descriptor: bv_pileup_token's layout (include/basevar_amd_pileup.h)
struct bv_tt_token {
    uint32_t pos, sample;
    uint64_t text_off;
    uint32_t text_len, reserved_;
};

struct bv_tt_carry {
    uint32_t fld;        // field of the step's first byte
    uint32_t tok;        // index, in its column, of the token that the step's first byte belongs to (or ends)
    uint32_t prev_sep;   // the byte before the step is a separator (the row's first step: 1)
    uint32_t open;       // the byte before the step is text of an indel token
    uint32_t n_tok;      // indel tokens begun before the step
    uint32_t n_txt;      // text bytes before the step
    uint32_t start_txt;  // n_txt at the first byte of the last token begun before the step (read while `open`)
};

struct bv_tt_masks {
    uint64_t M, IS, EN;
};

BV_TT_FN bv_tt_carry bv_tt_carry_init() {
    bv_tt_carry c;
    c.fld = 0; c.tok = 0; c.prev_sep = 1; c.open = 0; c.n_tok = 0; c.n_txt = 0; c.start_txt = 0;
    return c;
}

BV_TT_FN uint32_t bv_tt_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}
BV_TT_FN uint32_t bv_tt_top(uint64_t x) {  // index of the highest set bit, x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 63u - (uint32_t)__clzll((long long)x);
#else
    return 63u - (uint32_t)__builtin_clzll(x);
#endif
}
BV_TT_FN uint64_t bv_tt_below(uint32_t k) { return ((uint64_t)1 << k) - 1u; }  // bits 0 .. k-1, k < 64

// field of the byte at k (a tab belongs to the field it ends)
BV_TT_FN uint32_t bv_tt_field_at(const bv_tt_carry &c, uint64_t T, uint32_t k) { return c.fld + bv_tt_popc(T & bv_tt_below(k)); }

// index in its column of the token that the byte at k belongs to
BV_TT_FN uint32_t bv_tt_tok_at(const bv_tt_carry &c, uint64_t T, uint64_t S, uint32_t k) {
    const uint64_t lt = bv_tt_below(k), tb = T & lt;
    if (tb) return bv_tt_popc(S & lt & ~(((uint64_t)2 << bv_tt_top(tb)) - 1u));
    return c.tok + bv_tt_popc(S & lt);
}

// A run of non-separator bytes is token text <=> its first byte is an indel start, or it goes on a token open at the step's
// first byte.  Adding the starts to the mask of non-separators carries through exactly the runs that have one.
BV_TT_FN bv_tt_masks bv_tt_step_masks(const bv_tt_carry &c, uint64_t SEP, uint64_t V, uint64_t F5, uint64_t PM) {
    bv_tt_masks m;
    const uint64_t N = V & ~SEP;
    const uint64_t first = N & ((SEP << 1) | (uint64_t)(c.prev_sep & 1u));  // first bytes of tokens
    m.IS = first & PM & F5;
    const uint64_t from = m.IS | (N & (uint64_t)(c.open & 1u));
    m.M = N & ~(N + from);
    m.EN = SEP & V & ((m.M << 1) | (uint64_t)(c.open & 1u));
    return m;
}

// the byte at k is token text (M bit k): its place in the row's text
BV_TT_FN uint32_t bv_tt_text_at(const bv_tt_carry &c, const bv_tt_masks &m, uint32_t k) { return c.n_txt + bv_tt_popc(m.M & bv_tt_below(k)); }
// the byte at k begins a token (IS bit k): the token's ordinal in the row; its text begins at bv_tt_text_at(k)
BV_TT_FN uint32_t bv_tt_start_ord_at(const bv_tt_carry &c, const bv_tt_masks &m, uint32_t k) { return c.n_tok + bv_tt_popc(m.IS & bv_tt_below(k)); }
// the byte at k ends a token (EN bit k): the token's ordinal (it began before k: in the step or before it) ...
BV_TT_FN uint32_t bv_tt_end_ord_at(const bv_tt_carry &c, const bv_tt_masks &m, uint32_t k) { return c.n_tok + bv_tt_popc(m.IS & bv_tt_below(k)) - 1u; }
// ... and its length
BV_TT_FN uint32_t bv_tt_end_len_at(const bv_tt_carry &c, const bv_tt_masks &m, uint32_t k) {
    const uint64_t lt = bv_tt_below(k), sb = m.IS & lt;
    if (sb) return bv_tt_popc(m.M & lt & ~bv_tt_below(bv_tt_top(sb)));
    return c.n_txt + bv_tt_popc(m.M & lt) - c.start_txt;
}

// the carry of the next step
BV_TT_FN bv_tt_carry bv_tt_carry_next(const bv_tt_carry &c, const bv_tt_masks &m, uint64_t T, uint64_t S, uint64_t SEP) {
    bv_tt_carry n = c;
    if (m.IS) n.start_txt = c.n_txt + bv_tt_popc(m.M & bv_tt_below(bv_tt_top(m.IS)));
    n.n_tok = c.n_tok + bv_tt_popc(m.IS);
    n.n_txt = c.n_txt + bv_tt_popc(m.M);
    n.open = (uint32_t)(m.M >> 63);
    n.prev_sep = (uint32_t)(SEP >> 63);
    n.fld = c.fld + bv_tt_popc(T);
    if (T) {
        const uint32_t t = bv_tt_top(T);
        n.tok = t == 63u ? 0u : bv_tt_popc(S & ~(((uint64_t)2 << t) - 1u));
    } else {
        n.tok = c.tok + bv_tt_popc(S);
    }
    return n;
}

// Readbases is behind the step and no token is open: nothing more of the row is token text
BV_TT_FN bool bv_tt_done(const bv_tt_carry &c) { return c.fld > BV_TT_FIELD && !c.open; }

// The walk without a schedule: row[0 .. len) in steps of 64 bytes from its first byte, every byte of a step in turn.  tok (may
// be NULL: count only) takes the row's descriptors from tok[0], text_off counted from the row's first text byte; text (may be
// NULL) takes the text.  Returns the tokens, *n_txt the text bytes.
inline uint32_t bv_tt_row_serial(const char *row, uint32_t len, uint32_t pos, uint32_t sample0, bv_tt_token *tok, uint8_t *text, uint32_t *n_txt) {
    bv_tt_carry c = bv_tt_carry_init();
    for (uint32_t b = 0; b < len && !bv_tt_done(c); b += 64u) {
        uint64_t T = 0, S = 0, SEP = 0, V = 0, F5 = 0, PM = 0;
        for (uint32_t k = 0; k < 64u && b + k < len; ++k) {
            const char ch = row[b + k];
            const uint64_t bit = (uint64_t)1 << k;
            V |= bit;
            if (ch == '\t') T |= bit;
            if (ch == ' ') S |= bit;
            if (ch == '\t' || ch == ' ' || ch == '\n') SEP |= bit;
            if (ch == '+' || ch == '-') PM |= bit;
        }
        for (uint32_t k = 0; k < 64u; ++k)
            if (bv_tt_field_at(c, T, k) == BV_TT_FIELD) F5 |= (uint64_t)1 << k;
        const bv_tt_masks m = bv_tt_step_masks(c, SEP, V, F5, PM);
        for (uint32_t k = 0; k < 64u; ++k) {
            const uint64_t bit = (uint64_t)1 << k;
            if ((m.M & bit) && text) text[bv_tt_text_at(c, m, k)] = (uint8_t)row[b + k];
            if ((m.IS & bit) && tok) {
                bv_tt_token &t = tok[bv_tt_start_ord_at(c, m, k)];
                t.pos = pos; t.sample = sample0 + bv_tt_tok_at(c, T, S, k); t.text_off = bv_tt_text_at(c, m, k); t.reserved_ = 0;
            }
            if ((m.EN & bit) && tok) tok[bv_tt_end_ord_at(c, m, k)].text_len = bv_tt_end_len_at(c, m, k);
        }
        c = bv_tt_carry_next(c, m, T, S, SEP);
    }
    *n_txt = c.n_txt;
    return c.n_tok;
}
