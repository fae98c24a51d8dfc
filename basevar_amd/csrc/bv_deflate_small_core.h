// bv_deflate_small_core.h -- the second, opt-in level of the device DEFLATE encoder (BV_DEFLATE_SMALL of
// bv_engine_bgzf_deflate_level, include/basevar_amd_bgzf.h): dynamic Huffman codes over a parse that looks for 16-, 8- and
// 4-byte grams.  Written as bv_deflate_core.h is, whose chunk matcher, symbol mapping, bit buffer and member frame it uses:
// inline functions that the device kernel (bv_deflate.hip) and a plain g++ harness (tests/cpp/deflate_core_check.cpp --level
// small, run under ASan + UBSan) both compile; `nlanes` lanes execute it, `lane` only selects which part of a wide step a lane
// does, the CPU runs it as lane 0 of 1.
//
// One wave codes one block of 1 .. 0xff00 bytes into one whole BGZF member, a single final block, at most its text + 31 bytes.
//
// THE BYTES DEPEND ON THE TEXT ONLY.  What is coded is defined without reference to lanes:
//
// PARSE.  For g in {4, 8, 16}:
//   hash_g(p)  folds the g bytes at p as little-endian 32-bit words w0, w1, ...: v = 0; v = v * K + w_k (mod 2^32) in order,
//              K = 2654435761; then h = (v * K mod 2^32) >> (32 - 12).  For g = 4 this is bv_def_hash.
//   cand_g(p)  the largest q < p with hash_g(q) == hash_g(p), both with g bytes inside the block.  Every position enters every
//              table, positions inside a taken match too.
//   len_g(p)   the common prefix of text[p ..) and text[cand_g(p) ..), at most min(258, n - p).
//   The match at p belongs to the first g, in the order 16, 8, 4, for which cand_g(p) exists, p - cand_g(p) <= 32768 and
//   len_g(p) >= g.  If there is none, text[p] is a literal.  The parse is greedy from p = 0: a match is taken whole.
//
// COUNTS.  Literal/length symbols 0 .. 285 (256, the end code, counts once), distance symbols 0 .. 29.
//
// CODE LENGTHS of an alphabet with limit L (15 for the two alphabets above, 7 for the code-length alphabet):
//   1  while fewer than two symbols have a non-zero count, the lowest-numbered symbol whose count is 0 gets count 1 (a block
//      without matches gets the distance lengths [1, 1], which every inflater accepts);
//   2  the symbols with non-zero count are sorted ascending by (count, symbol) and the Huffman tree is built with two queues,
//      the sorted leaves and the internal nodes in the order of their creation: each step takes the two lightest heads, on
//      equal weight the leaf before the internal node.  Length = depth;
//   3  if the deepest leaf is deeper than L, every non-zero count c becomes (c + 1) / 2 (integer division) and 2 is repeated.
//      The number of such rounds is part of the definition (bv_defs_code_lengths returns it).
//   Canonical codes follow RFC 1951 3.2.2.
//
// BLOCK HEADER.  HLIT = max(257, 1 + the last literal/length symbol with a length), HDIST = max(1, 1 + the last distance
//   symbol with one).  The two length lists are joined into one sequence and spelled greedily from i = 0, with v = seq[i] and
//   r = the run of v that starts at i (runs may cross from the literal into the distance lengths):
//     v == 0 and r >= 3                              symbol 17 for r (r <= 10), else symbol 18 for min(r, 138)
//     v != 0, i > 0, seq[i - 1] == v and r >= 3      symbol 16 for min(r, 6)
//     else                                           v itself, one place
//   The code-length alphabet's lengths come from the construction above with L = 7, and
//   HCLEN = max(4, 1 + the last non-zero in the order 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15).
//
// CHOICE.  The same tokens give three payloads: stored (5 + n bytes), fixed codes, dynamic codes.  Dynamic is chosen if its
//   bytes are fewer than the fixed form's and fewer than 5 + n; else fixed, if fewer than 5 + n; else stored.  All three
//   sizes follow from the counts before a bit is written, and only the chosen form is written.
//
// A serial coder computes exactly this (tests/deflate_small_model.py is one, written from these lines).  Here the parse runs
// BV_DEF_CHUNK positions at a time through bv_deflate_core.h's bv_def_chunk, with three tables; the tokens leave the parse 64 at a time for a
// run of the caller's (`tok`: device memory on the device, one 256-byte store per 64 tokens) and are counted as they leave;
// one lane builds the trees (a few hundred steps per alphabet; the sort before them is shared); the codes are written 64
// tokens at a time: every lane looks up its token's bits, the bit counts are summed in front of it, and the bits are ORed
// into a zeroed window whose whole words then leave for the member.
#ifndef BV_DEFLATE_SMALL_CORE_H
#define BV_DEFLATE_SMALL_CORE_H

#include "bv_deflate_core.h"

#define BV_DEFS_NLL 286u
#define BV_DEFS_ND 30u
#define BV_DEFS_NCL 19u
#define BV_DEFS_MAX_SYMS 286u
#define BV_DEFS_SEQ (BV_DEFS_NLL + BV_DEFS_ND)
#define BV_DEFS_TOK_MATCH 0x80000000u  // a token: a literal's byte (256: the end code), or this | (length - 3) << 15 | (distance - 1)
#define BV_DEFS_WIN_WORDS 104u         // 31 bits carried + 64 tokens of at most 48 bits, and the two words a token's OR may touch behind
#define BV_DEFS_FORM_STORED 0u
#define BV_DEFS_FORM_FIXED 1u
#define BV_DEFS_FORM_DYNAMIC 2u

// tokens a block of n bytes needs room for in `tok`: every byte a literal, the end code, rounded to whole stores
#define BV_DEFS_TOK_ROOM(n) ((((n) + 1u) + 63u) & ~63u)

#if defined(__HIP_DEVICE_COMPILE__)
#define BV_DEFS_ADD(p, v) (void)atomicAdd((p), (v))
#define BV_DEFS_OR(p, v) (void)atomicOr((p), (v))
#else
#define BV_DEFS_ADD(p, v) (void)(*(p) += (v))
#define BV_DEFS_OR(p, v) (void)(*(p) |= (v))
#endif

// the workspace of the code-length construction (LDS on the device)
struct BvDefsHuff {
    uint32_t w[BV_DEFS_MAX_SYMS];           // the counts as the rounds leave them
    uint16_t order[BV_DEFS_MAX_SYMS];       // the symbols with a count, ascending by (count, symbol)
    uint32_t weight[2 * BV_DEFS_MAX_SYMS];  // the nodes: the leaves in that order, then the internal nodes as they were made
    uint16_t parent[2 * BV_DEFS_MAX_SYMS];
    uint16_t depth[2 * BV_DEFS_MAX_SYMS];
    uint16_t next[16];                      // RFC 1951 3.2.2: the next code of every length
    uint32_t nleaf, deepest;
};

// State of one block: 24 KiB of tables + 11.5 KiB (LDS on the device).
struct BvDefSmallState {
    BvDefMatch<3> M;                  // the grams of 4, 8 and 16 bytes
    uint32_t tokbuf[64];              // tokens on their way out
    uint32_t ll_cnt[BV_DEFS_NLL], d_cnt[BV_DEFS_ND + 2u], cl_cnt[BV_DEFS_NCL + 1u];
    uint8_t ll_len[BV_DEFS_NLL + 2u], d_len[BV_DEFS_ND + 2u], cl_len[BV_DEFS_NCL + 1u];
    uint16_t ll_code[BV_DEFS_NLL + 2u], d_code[BV_DEFS_ND + 2u], cl_code[BV_DEFS_NCL + 1u];  // as they enter the stream: reversed
    uint8_t seq[BV_DEFS_SEQ], cl_sym[BV_DEFS_SEQ], cl_ext[BV_DEFS_SEQ];
    uint32_t n_cl, hlit, hdist, hclen, form, plen;
    uint64_t ecode[64];               // a batch's bits per token
    uint8_t ebits[64];                // ... and how many
    uint32_t ewin[BV_DEFS_WIN_WORDS];
    BvDefsHuff H;
};

BV_DEF_FN uint32_t bv_defs_cl_order(uint32_t k) { return (uint32_t)"\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f"[k]; }

// the extra bits of a length and of a distance symbol (RFC 1951 3.2.5)
BV_DEF_FN uint32_t bv_defs_len_extra_bits(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) / 4u; }
BV_DEF_FN uint32_t bv_defs_dist_extra_bits(uint32_t sym) { return sym < 4u ? 0u : (sym - 2u) / 2u; }

// The code lengths of counts[0 .. nsym) with limit L, 2 <= nsym <= BV_DEFS_MAX_SYMS <= 2^L... (nsym <= 2^limit: the rounds end when
// every count is 1 at the latest, and equal counts give a tree of depth ceil(log2)); the counts add up to less than 2^32.
// len[0 .. nsym) is written; returns the rounds of step 3.  All lanes call it; the value is the same in every lane.
BV_DEF_FN uint32_t bv_defs_code_lengths(const uint32_t *counts, uint32_t nsym, uint32_t limit, uint8_t *len, BvDefsHuff *H, uint32_t lane, uint32_t nlanes) {
    for (uint32_t i = lane; i < nsym; i += nlanes) { H->w[i] = counts[i]; len[i] = 0; }
    BV_DEF_WAVE_SYNC();
    if (lane == 0) {
        uint32_t nz = 0;
        for (uint32_t i = 0; i < nsym; ++i) nz += H->w[i] != 0;
        for (uint32_t i = 0; i < nsym && nz < 2u; ++i)
            if (H->w[i] == 0) { H->w[i] = 1u; ++nz; }
        H->nleaf = nz;
    }
    BV_DEF_WAVE_SYNC();
    const uint32_t m = H->nleaf;
    uint32_t rounds = 0;
    for (;;) {
        // the sort: every symbol counts those before it
        for (uint32_t i = lane; i < nsym; i += nlanes) {
            const uint32_t c = H->w[i];
            if (c == 0) continue;
            uint32_t r = 0;
            for (uint32_t j = 0; j < nsym; ++j) {
                const uint32_t cj = H->w[j];
                r += (cj != 0 && (cj < c || (cj == c && j < i))) ? 1u : 0u;
            }
            H->order[r] = (uint16_t)i;
            H->weight[r] = c;
        }
        BV_DEF_WAVE_SYNC();
        if (lane == 0) {
            uint32_t li = 0, ii = m, nn = m;  // the heads of the two queues, the node to be made
            while (nn < 2u * m - 1u) {
                uint32_t sum = 0;
                for (uint32_t t = 0; t < 2u; ++t) {
                    uint32_t pick;
                    if (li < m && (ii >= nn || H->weight[li] <= H->weight[ii])) pick = li++;
                    else pick = ii++;
                    sum += H->weight[pick];
                    H->parent[pick] = (uint16_t)nn;
                }
                H->weight[nn] = sum;
                ++nn;
            }
            H->depth[2u * m - 2u] = 0;
            uint32_t deepest = 0;
            for (uint32_t k = 2u * m - 2u; k-- > 0;) {
                const uint32_t d = (uint32_t)H->depth[H->parent[k]] + 1u;
                H->depth[k] = (uint16_t)d;
                if (k < m && d > deepest) deepest = d;
            }
            H->deepest = deepest;
        }
        BV_DEF_WAVE_SYNC();
        if (H->deepest <= limit) break;
        ++rounds;
        for (uint32_t i = lane; i < nsym; i += nlanes) {
            const uint32_t c = H->w[i];
            if (c) H->w[i] = c / 2u + (c & 1u);
        }
        BV_DEF_WAVE_SYNC();
    }
    for (uint32_t k = lane; k < m; k += nlanes) len[H->order[k]] = (uint8_t)H->depth[k];
    BV_DEF_WAVE_SYNC();
    return rounds;
}

// RFC 1951 3.2.2, the codes reversed as they enter the stream.  One lane's work.
BV_DEF_FN void bv_defs_codes(const uint8_t *len, uint32_t nsym, uint16_t *code, BvDefsHuff *H, uint32_t lane) {
    if (lane == 0) {
        for (uint32_t b = 0; b < 16u; ++b) H->next[b] = 0;
        for (uint32_t s = 0; s < nsym; ++s) H->next[len[s]] += 1u;
        uint32_t c = 0, before = 0;  // (the count of length 0 does not enter)
        for (uint32_t b = 1; b < 16u; ++b) {
            c = (c + before) << 1;
            before = H->next[b];
            H->next[b] = (uint16_t)c;
        }
        for (uint32_t s = 0; s < nsym; ++s) {
            const uint32_t l = len[s];
            code[s] = 0;
            if (l) { code[s] = (uint16_t)bv_def_rev(H->next[l], l); H->next[l] += 1u; }
        }
    }
    BV_DEF_WAVE_SYNC();
}

// 64 tokens (m of them) leave S->tokbuf for tok[at ..) and are counted
BV_DEF_FN void bv_defs_flush(BvDefSmallState *S, uint32_t *tok, uint32_t at, uint32_t m, uint32_t lane, uint32_t nlanes) {
    BV_DEF_WAVE_SYNC();
    for (uint32_t i = lane; i < m; i += nlanes) {
        const uint32_t t = S->tokbuf[i];
        tok[at + i] = t;
        if (t & BV_DEFS_TOK_MATCH) {
            uint32_t sym, eb, extra;
            bv_def_len_sym((t >> 15) & 0xffu, sym, eb, extra);
            BV_DEFS_ADD(&S->ll_cnt[sym], 1u);
            bv_def_dist_sym(t & 0x7fffu, sym, eb, extra);
            BV_DEFS_ADD(&S->d_cnt[sym], 1u);
        } else {
            BV_DEFS_ADD(&S->ll_cnt[t], 1u);
        }
    }
    BV_DEF_WAVE_SYNC();
}

// The parse of text[0 .. n): the tokens to tok[0 ..), the end code behind them, the counts to S.  Returns the number of tokens.
BV_DEF_FN uint32_t bv_defs_parse(const uint8_t *text, uint32_t n, BvDefSmallState *S, uint32_t *tok, uint32_t lane, uint32_t nlanes) {
    for (uint32_t i = lane; i < BV_DEFS_NLL; i += nlanes) S->ll_cnt[i] = 0;
    for (uint32_t i = lane; i < BV_DEFS_ND + 2u; i += nlanes) S->d_cnt[i] = 0;
    bv_def_clear(&S->M, lane, nlanes);
    uint32_t cur = 0, ntok = 0;
    for (uint32_t base = 0; base < n; base += BV_DEF_CHUNK) {
        bv_def_chunk(text, n, base, cur, &S->M, lane, nlanes);
        const uint32_t end = base + BV_DEF_CHUNK < n ? base + BV_DEF_CHUNK : n;
        while (cur < end) {
            const uint32_t i = cur - base, len = S->M.len[i];
            uint32_t t;
            if (len) {
                t = BV_DEFS_TOK_MATCH | ((len - 3u) << 15) | (uint32_t)S->M.dist[i];
                cur += len;
            } else {
                t = text[cur];
                cur += 1u;
            }
            if (lane == 0) S->tokbuf[ntok & 63u] = t;
            ++ntok;
            if ((ntok & 63u) == 0) bv_defs_flush(S, tok, ntok - 64u, 64u, lane, nlanes);
        }
        BV_DEF_WAVE_SYNC();
    }
    if (lane == 0) S->tokbuf[ntok & 63u] = 256u;
    ++ntok;
    if (ntok & 63u) bv_defs_flush(S, tok, ntok & ~63u, ntok & 63u, lane, nlanes);
    else bv_defs_flush(S, tok, ntok - 64u, 64u, lane, nlanes);
    return ntok;
}

// From the counts: the three code tables, the header's spelling, the three sizes and the choice (S->form, S->plen: the
// payload's bytes).  Leaves S->ll_len / ll_code / d_len / d_code as the chosen form codes with them.
BV_DEF_FN void bv_defs_plan(uint32_t n, BvDefSmallState *S, uint32_t lane, uint32_t nlanes) {
    bv_defs_code_lengths(S->ll_cnt, BV_DEFS_NLL, 15u, S->ll_len, &S->H, lane, nlanes);
    bv_defs_code_lengths(S->d_cnt, BV_DEFS_ND, 15u, S->d_len, &S->H, lane, nlanes);
    if (lane == 0) {
        uint32_t hlit = 257u, hdist = 1u;
        for (uint32_t s = 257u; s < BV_DEFS_NLL; ++s)
            if (S->ll_len[s]) hlit = s + 1u;
        for (uint32_t s = 1u; s < BV_DEFS_ND; ++s)
            if (S->d_len[s]) hdist = s + 1u;
        for (uint32_t s = 0; s < hlit; ++s) S->seq[s] = S->ll_len[s];
        for (uint32_t s = 0; s < hdist; ++s) S->seq[hlit + s] = S->d_len[s];
        for (uint32_t s = 0; s < BV_DEFS_NCL + 1u; ++s) S->cl_cnt[s] = 0;
        const uint32_t total = hlit + hdist;
        uint32_t ncl = 0;
        for (uint32_t i = 0; i < total;) {
            const uint32_t v = S->seq[i], most = v == 0 ? 138u : 6u;  // (no decision looks at more of a run)
            uint32_t r = 1u, sym = v, ext = 0, adv = 1u;
            while (r < most && i + r < total && S->seq[i + r] == v) ++r;
            if (v == 0 && r >= 3u) {
                if (r <= 10u) { sym = 17u; ext = r - 3u; }
                else { sym = 18u; ext = r - 11u; }
                adv = r;
            } else if (v != 0 && i > 0 && S->seq[i - 1u] == v && r >= 3u) {
                sym = 16u; ext = r - 3u; adv = r;
            }
            S->cl_sym[ncl] = (uint8_t)sym; S->cl_ext[ncl] = (uint8_t)ext;
            S->cl_cnt[sym] += 1u;
            ++ncl;
            i += adv;
        }
        S->n_cl = ncl; S->hlit = hlit; S->hdist = hdist;
    }
    BV_DEF_WAVE_SYNC();
    bv_defs_code_lengths(S->cl_cnt, BV_DEFS_NCL, 7u, S->cl_len, &S->H, lane, nlanes);
    if (lane == 0) {
        uint32_t hclen = 4u;
        for (uint32_t k = 4u; k < BV_DEFS_NCL; ++k)
            if (S->cl_len[bv_defs_cl_order(k)]) hclen = k + 1u;
        uint32_t dyn = 3u + 14u + 3u * hclen, fix = 3u, extra = 0;
        for (uint32_t s = 0; s < BV_DEFS_NCL; ++s) dyn += S->cl_cnt[s] * ((uint32_t)S->cl_len[s] + (s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u));
        for (uint32_t s = 0; s < BV_DEFS_NLL; ++s) {
            const uint32_t c = S->ll_cnt[s];
            dyn += c * S->ll_len[s]; fix += c * bv_def_fixed_len(s); extra += c * bv_defs_len_extra_bits(s);
        }
        for (uint32_t s = 0; s < BV_DEFS_ND; ++s) {
            const uint32_t c = S->d_cnt[s];
            dyn += c * S->d_len[s]; fix += c * 5u; extra += c * bv_defs_dist_extra_bits(s);
        }
        const uint32_t dyn_bytes = (dyn + extra + 7u) / 8u, fix_bytes = (fix + extra + 7u) / 8u, stored = 5u + n;
        S->hclen = hclen;
        if (dyn_bytes < fix_bytes && dyn_bytes < stored) { S->form = BV_DEFS_FORM_DYNAMIC; S->plen = dyn_bytes; }
        else if (fix_bytes < stored) { S->form = BV_DEFS_FORM_FIXED; S->plen = fix_bytes; }
        else { S->form = BV_DEFS_FORM_STORED; S->plen = stored; }
    }
    BV_DEF_WAVE_SYNC();
    if (S->form == BV_DEFS_FORM_DYNAMIC) {
        bv_defs_codes(S->ll_len, BV_DEFS_NLL, S->ll_code, &S->H, lane);
        bv_defs_codes(S->d_len, BV_DEFS_ND, S->d_code, &S->H, lane);
        bv_defs_codes(S->cl_len, BV_DEFS_NCL, S->cl_code, &S->H, lane);
    } else if (S->form == BV_DEFS_FORM_FIXED) {
        for (uint32_t s = lane; s < BV_DEFS_NLL; s += nlanes) {
            const uint32_t l = bv_def_fixed_len(s);
            S->ll_len[s] = (uint8_t)l; S->ll_code[s] = (uint16_t)bv_def_rev(bv_def_fixed_code(s), l);
        }
        for (uint32_t s = lane; s < BV_DEFS_ND; s += nlanes) { S->d_len[s] = 5u; S->d_code[s] = (uint16_t)bv_def_rev(s, 5); }
        BV_DEF_WAVE_SYNC();
    }
}

// The chosen form (fixed or dynamic) of the ntok tokens, from out + 18 on: S->plen bytes.
BV_DEF_FN void bv_defs_emit(uint8_t *out, const uint32_t *tok, uint32_t ntok, BvDefSmallState *S, uint32_t lane, uint32_t nlanes) {
    BvDefBits b;
    b.out = out + 16; b.pos = 0; b.limit = 2u + S->plen; b.cnt = 16u; b.over = 0; b.buf = 0;
    bv_def_put(b, 1u | (S->form << 1), 3, lane);  // BFINAL = 1, BTYPE
    if (S->form == BV_DEFS_FORM_DYNAMIC) {
        bv_def_put(b, S->hlit - 257u, 5, lane);
        bv_def_put(b, S->hdist - 1u, 5, lane);
        bv_def_put(b, S->hclen - 4u, 4, lane);
        for (uint32_t k = 0; k < S->hclen; ++k) bv_def_put(b, S->cl_len[bv_defs_cl_order(k)], 3, lane);
        const uint32_t ncl = S->n_cl;
        for (uint32_t k = 0; k < ncl; ++k) {
            const uint32_t sym = S->cl_sym[k];
            bv_def_put(b, S->cl_code[sym], S->cl_len[sym], lane);
            if (sym >= 16u) bv_def_put(b, S->cl_ext[k], sym == 16u ? 2u : sym == 17u ? 3u : 7u, lane);
        }
    }
    // the tokens, 64 at a time, through a window of whole words; word 0 holds the bits that have not filled a word yet
    uint32_t pos = b.pos, cnt = b.cnt;
    for (uint32_t k = lane; k < BV_DEFS_WIN_WORDS; k += nlanes) S->ewin[k] = k == 0 ? (uint32_t)b.buf : 0u;
    BV_DEF_WAVE_SYNC();
    for (uint32_t base = 0; base < ntok; base += 64u) {
        const uint32_t m = ntok - base < 64u ? ntok - base : 64u;
        for (uint32_t i = lane; i < 64u; i += nlanes) {
            uint64_t code = 0;
            uint32_t nb = 0;
            if (i < m) {
                const uint32_t t = tok[base + i];
                if (t & BV_DEFS_TOK_MATCH) {
                    uint32_t sym, eb, extra;
                    bv_def_len_sym((t >> 15) & 0xffu, sym, eb, extra);
                    code = S->ll_code[sym]; nb = S->ll_len[sym];
                    code |= (uint64_t)extra << nb; nb += eb;
                    bv_def_dist_sym(t & 0x7fffu, sym, eb, extra);
                    code |= (uint64_t)S->d_code[sym] << nb; nb += S->d_len[sym];
                    code |= (uint64_t)extra << nb; nb += eb;
                } else {
                    code = S->ll_code[t]; nb = S->ll_len[t];
                }
            }
            S->ecode[i] = code;
            S->ebits[i] = (uint8_t)nb;
        }
        BV_DEF_WAVE_SYNC();
        uint32_t total = cnt;
        for (uint32_t i = lane; i < 64u; i += nlanes) {
            uint32_t at = cnt;
            total = cnt;
            for (uint32_t j = 0; j < 64u; ++j) {
                const uint32_t nb = S->ebits[j];
                if (j < i) at += nb;
                total += nb;
            }
            const uint64_t code = S->ecode[i];
            if (S->ebits[i]) {
                const uint32_t w = at >> 5, sh = at & 31u;
                const uint64_t lo = code << sh;
                BV_DEFS_OR(&S->ewin[w], (uint32_t)lo);
                if ((uint32_t)(lo >> 32)) BV_DEFS_OR(&S->ewin[w + 1u], (uint32_t)(lo >> 32));
                if (sh && (uint32_t)(code >> (64u - sh))) BV_DEFS_OR(&S->ewin[w + 2u], (uint32_t)(code >> (64u - sh)));
            }
        }
        BV_DEF_WAVE_SYNC();
        const uint32_t full = total >> 5;
        for (uint32_t k = lane; k < full; k += nlanes) {
            if (pos + 4u * k + 4u > b.limit) continue;  // (never: the sizes were counted)
            bv_def_store_word(b.out + pos + 4u * k, S->ewin[k]);
        }
        const uint32_t carry = S->ewin[full];
        BV_DEF_WAVE_SYNC();
        for (uint32_t k = lane; k <= full + 2u && k < BV_DEFS_WIN_WORDS; k += nlanes) S->ewin[k] = k == 0 ? carry : 0u;
        BV_DEF_WAVE_SYNC();
        pos += 4u * full;
        cnt = total & 31u;
    }
    if (lane == 0) {
        const uint32_t w = S->ewin[0];
        for (uint32_t k = 0; k * 8u < cnt && pos + k < b.limit; ++k) b.out[pos + k] = (uint8_t)(w >> (8u * k));
    }
}

// One whole BGZF member of text[0 .. n), 1 <= n <= BV_DEF_MAX_BLOCK, at `out` (room for n + BV_DEF_MEMBER_EXTRA bytes; 4-byte
// aligned on the device), as bv_def_member.  tok: room for BV_DEFS_TOK_ROOM(n) tokens.  Returns the member's bytes.
template <class Reduce>
BV_DEF_FN uint32_t bv_def_small_member(const uint8_t *text, uint32_t n, uint8_t *out, BvDefSmallState *S, uint32_t *tok, const uint32_t *crc_tab,
                                       uint32_t lane, uint32_t nlanes, Reduce crc_reduce) {
    const uint32_t ntok = bv_defs_parse(text, n, S, tok, lane, nlanes);
    bv_defs_plan(n, S, lane, nlanes);
    if (S->form != BV_DEFS_FORM_STORED) bv_defs_emit(out, tok, ntok, S, lane, nlanes);
    return bv_def_frame(text, n, out, S->form == BV_DEFS_FORM_STORED ? 0u : S->plen, crc_tab, lane, nlanes, crc_reduce);
}

#endif  // BV_DEFLATE_SMALL_CORE_H
