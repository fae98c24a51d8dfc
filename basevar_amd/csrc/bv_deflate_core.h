// bv_deflate_core.h -- the DEFLATE (RFC 1951) encoder behind bv_engine_bgzf_deflate (include/basevar_amd_bgzf.h), as inline
// functions that the device kernel (bv_deflate.hip) and a plain g++ harness (tests/cpp/deflate_core_check.cpp, run under
// ASan + UBSan) both compile; the mirror of bv_inflate_core.h and written the same way: `nlanes` lanes execute it, `lane`
// only selects which part of a wide step a lane does, the CPU runs it as lane 0 of 1.
//
// One wave codes one block of 1 .. 0xff00 bytes of text into one whole BGZF member: 18-byte header, one raw DEFLATE stream,
// CRC32, ISIZE.  The stream is a single final block, either LZ77 + the fixed Huffman codes or stored, whichever is smaller
// (stored on a tie), so a member never exceeds 18 + 5 + 0xff00 + 8 bytes.
//
// THE BYTES DEPEND ON THE TEXT ONLY.  What is coded is defined without reference to lanes:
//   cand(p)  = the largest q < p with hash(text[q .. q+4)) == hash(text[p .. p+4))      (both with 4 bytes inside the block)
//   len(p)   = the common prefix of text[p ..) and text[cand(p) ..), at most min(258, n - p); a match if it is >= 4 and
//              p - cand(p) <= 32768
//   the parse is greedy from p = 0: a match at p is taken whole, else text[p] is a literal.
// A serial coder with a head-of-chain hash table computes exactly this (tests/deflate_model.py is one, written from these lines;
// the tests hold this file's members to its bytes).  Here the positions are handled BV_DEF_CHUNK at a
// time, in steps that are separated by BV_DEF_WAVE_SYNC and are data-parallel inside:
//   1  every position of the chunk reads the table as the chunks before left it and posts its hash;
//   2  ... takes the nearest earlier position of its own chunk with the same hash in its place, if there is one (so a match at
//      a distance shorter than the chunk is found: `\t./.` repeated is most of a VCF line), notes whether a later one exists,
//      and measures its match;
//   3  the last position of every hash in the chunk -- one writer per entry, no race -- enters the table;
//   4  all lanes walk the parse with the same values and append the codes to one bit buffer; lane 0 stores it.
// cand() of a position does not depend on where chunks begin, so neither do the bytes.  Positions that the parse cursor has
// already passed when their chunk begins (the cursor is part of the parse, not of the schedule) are not measured.
#ifndef BV_DEFLATE_CORE_H
#define BV_DEFLATE_CORE_H

#include <stdint.h>
#include <string.h>

#include "bv_inflate_core.h"  // the CRC32 tables and shares, BV_INF_WAVE_SYNC

#define BV_DEF_FN BV_INF_FN
#define BV_DEF_WAVE_SYNC() BV_INF_WAVE_SYNC()

#define BV_DEF_MAX_BLOCK 0xff00u   // text bytes per member (what htslib and host/bgzf_tabix.hpp cut)
#define BV_DEF_MEMBER_EXTRA 31u    // 18 header + 5 stored-block header + 8 trailer: a member is at most its text + this
#define BV_DEF_MIN_MATCH 4u
#define BV_DEF_MAX_MATCH 258u
#define BV_DEF_WINDOW 32768u
#ifndef BV_DEF_HASH_BITS
#define BV_DEF_HASH_BITS 12u
#endif
#define BV_DEF_CHUNK 64u
#define BV_DEF_NO_HASH 0xffffu     // fewer bytes left than the gram has (a hash has BV_DEF_HASH_BITS bits)
#define BV_DEF_TEXT_PAD 8u         // bytes behind the text that the device's window must own (bv_def_load4 reads whole words)

// The chunk's hashes, 16 bits a gram from bit 0, 16, 32, one word a position: the compare loop of step 2 reads one word a step.
template <int NG> struct BvDefRow { typedef uint64_t type; };
template <> struct BvDefRow<1> { typedef uint16_t type; };
static_assert(BV_DEF_HASH_BITS <= 15u, "a hash is never BV_DEF_NO_HASH or 0xfffe, the two values of a 16-bit field that stand for no hash");

// Match state of one block over NG grams, gram k of 4 << k bytes: 8 KiB of table a gram + the chunk (LDS on the device).  The
// parse of this file has the one gram of 4 bytes; bv_deflate_small_core.h has three.
template <int NG> struct BvDefMatch {
    uint16_t head[NG][1u << BV_DEF_HASH_BITS];  // position + 1 of the latest position with this hash; 0: none
    typename BvDefRow<NG>::type hash[BV_DEF_CHUNK];  // the chunk's hashes (BV_DEF_NO_HASH: too few bytes left)
    uint16_t cand[NG][BV_DEF_CHUNK];            // position + 1 of the candidate from the table; 0: none
    uint16_t len[BV_DEF_CHUNK];                 // match length, 0: a literal
    uint16_t dist[BV_DEF_CHUNK];                // distance - 1
    uint8_t last[BV_DEF_CHUNK];                 // bit k: no later position of the chunk has this hash of gram k
};
typedef BvDefMatch<1> BvDefState;

// four bytes at any offset, little-endian.  The device reads the two aligned words around them (`text` is the 4-byte aligned
// LDS window, with BV_DEF_TEXT_PAD bytes behind the text); the host reads exactly the four.
BV_DEF_FN uint32_t bv_def_load4(const uint8_t *text, uint32_t p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t *w = reinterpret_cast<const uint32_t *>(text) + (p >> 2);
    const uint64_t v = ((uint64_t)w[1] << 32) | w[0];
    return (uint32_t)(v >> (8u * (p & 3u)));
#else
    uint32_t v;
    memcpy(&v, text + p, 4);
    return v;
#endif
}
BV_DEF_FN uint32_t bv_def_hash(uint32_t v) { return (v * 2654435761u) >> (32u - BV_DEF_HASH_BITS); }

// the common prefix of text[p ..) and text[q ..), at most maxl
BV_DEF_FN uint32_t bv_def_measure(const uint8_t *text, uint32_t p, uint32_t q, uint32_t maxl) {
    uint32_t len = 0;
    while (len + 4u <= maxl && bv_def_load4(text, p + len) == bv_def_load4(text, q + len)) len += 4u;
    while (len < maxl && text[p + len] == text[q + len]) ++len;
    return len;
}

// no position has entered a table
template <int NG> BV_DEF_FN void bv_def_clear(BvDefMatch<NG> *M, uint32_t lane, uint32_t nlanes) {
    for (uint32_t i = lane; i < (uint32_t)NG << BV_DEF_HASH_BITS; i += nlanes) (&M->head[0][0])[i] = 0;
    BV_DEF_WAVE_SYNC();
}

// Steps 1 to 3 of the chunk at `base` (the head of this file), for every gram: M->len / M->dist of its positions for the
// walk, which the caller does, and the tables as the next chunk finds them.  cur: the parse's cursor.  The match at a position
// belongs to the longest gram whose candidate exists, lies inside the window and repeats the whole gram.
template <int NG>
BV_DEF_FN void bv_def_chunk(const uint8_t *text, uint32_t n, uint32_t base, uint32_t cur, BvDefMatch<NG> *M, uint32_t lane, uint32_t nlanes) {
    typedef typename BvDefRow<NG>::type Row;
    const bool measure = cur < base + BV_DEF_CHUNK;  // else an earlier match covers the whole chunk: only the tables are kept
    for (uint32_t i = lane; i < BV_DEF_CHUNK; i += nlanes) {
        const uint32_t p = base + i;
        Row row = 0;
        uint32_t v = 0, words = 0;  // the fold of the gram's 32-bit words: v = v * K + w_k, hashed as a 4-gram's word is
        for (int k = 0; k < NG; ++k) {
            uint32_t h = BV_DEF_NO_HASH, c = 0;
            if (p + (4u << k) <= n) {
                for (; words < (1u << k); ++words) v = v * 2654435761u + bv_def_load4(text, p + 4u * words);
                h = bv_def_hash(v);
                c = M->head[k][h];
            }
            row |= (Row)h << (16 * k);
            M->cand[k][i] = (uint16_t)c;
        }
        M->hash[i] = row;
    }
    BV_DEF_WAVE_SYNC();
    for (uint32_t i = lane; i < BV_DEF_CHUNK; i += nlanes) {
        const uint32_t p = base + i;
        const Row mine = M->hash[i];
        uint32_t h[NG], c[NG], last = (1u << NG) - 1u, len = 0, from = 0;
        for (int k = 0; k < NG; ++k) {
            h[k] = (uint32_t)(mine >> (16 * k)) & 0xffffu;
            c[k] = M->cand[k][i];
            if (k > 0 && h[k] == BV_DEF_NO_HASH) h[k] = 0xfffeu;  // (a gram this position does not have matches nobody's: no hash is 0xfffe)
        }
        if (h[0] != BV_DEF_NO_HASH) {
            for (uint32_t j = 0; j < BV_DEF_CHUNK; ++j) {
                const Row x = M->hash[j];
                for (int k = 0; k < NG; ++k) {
                    const bool same = ((uint32_t)(x >> (16 * k)) & 0xffffu) == h[k];
                    if (same && j < i) c[k] = base + j + 1u;
                    if (same && j > i) last &= ~(1u << k);
                }
            }
        }
        if (measure && p >= cur && p < n) {
            const uint32_t maxl = n - p < BV_DEF_MAX_MATCH ? n - p : BV_DEF_MAX_MATCH;
            for (int k = NG - 1; k >= 0; --k) {
                if (len == 0 && c[k] != 0 && p - (c[k] - 1u) <= BV_DEF_WINDOW) {
                    len = bv_def_measure(text, p, c[k] - 1u, maxl);
                    from = c[k];
                    if (len < (4u << k)) len = 0;
                }
            }
        }
        M->last[i] = (uint8_t)last;
        M->len[i] = (uint16_t)len;
        M->dist[i] = (uint16_t)(len ? p - (from - 1u) - 1u : 0u);  // distance - 1: 0 .. 32767
    }
    BV_DEF_WAVE_SYNC();
    for (uint32_t i = lane; i < BV_DEF_CHUNK; i += nlanes) {
        const Row mine = M->hash[i];
        const uint32_t last = M->last[i];
        for (int k = 0; k < NG; ++k) {
            const uint32_t h = (uint32_t)(mine >> (16 * k)) & 0xffffu;
            if (h != BV_DEF_NO_HASH && ((last >> k) & 1u)) M->head[k][h] = (uint16_t)(base + i + 1u);
        }
    }
}

// a whole word of a coded stream, at a 4-byte aligned place on the device
BV_DEF_FN void bv_def_store_word(uint8_t *at, uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint32_t *>(at) = w;
#else
    memcpy(at, &w, 4);
#endif
}

// the bit buffer of the coded stream; the same in every lane.  Bytes leave it four at a time, at out + pos (4-byte aligned on
// the device: coding starts at out + 16 with the header's last two bytes as 16 bits that are overwritten later).
struct BvDefBits {
    uint8_t *out;
    uint32_t pos;    // bytes stored, from `out`
    uint32_t limit;  // a store that would pass out + limit is not made; `over` is set instead
    uint32_t cnt;    // bits in buf, < 32 between calls
    uint32_t over;
    uint64_t buf;
};
BV_DEF_FN void bv_def_put(BvDefBits &b, uint32_t bits, uint32_t n, uint32_t lane) {
    b.buf |= (uint64_t)bits << b.cnt;
    b.cnt += n;
    if (b.cnt >= 32u) {
        if (b.pos + 4u > b.limit) b.over = 1u;
        else if (lane == 0) bv_def_store_word(b.out + b.pos, (uint32_t)b.buf);
        b.pos += 4u;
        b.buf >>= 32;
        b.cnt -= 32u;
    }
}
// an n-bit Huffman code, which DEFLATE packs from its most significant bit
BV_DEF_FN uint32_t bv_def_rev(uint32_t code, uint32_t n) { return bv_inf_rev16(code) >> (16u - n); }

// RFC 1951 3.2.5 in closed form.  l = length - 3 (0 .. 255), d = distance - 1 (0 .. 32767)
BV_DEF_FN void bv_def_len_sym(uint32_t l, uint32_t &sym, uint32_t &eb, uint32_t &extra) {
    if (l == 255u) { sym = 285u; eb = 0; extra = 0; }
    else if (l < 8u) { sym = 257u + l; eb = 0; extra = 0; }
    else {
        eb = (31u - (uint32_t)__builtin_clz(l)) - 2u;
        sym = 261u + 4u * eb + ((l >> eb) & 3u);
        extra = l & ((1u << eb) - 1u);
    }
}
BV_DEF_FN void bv_def_dist_sym(uint32_t d, uint32_t &sym, uint32_t &eb, uint32_t &extra) {
    if (d < 4u) { sym = d; eb = 0; extra = 0; }
    else {
        eb = (31u - (uint32_t)__builtin_clz(d)) - 1u;
        sym = 2u * eb + 2u + ((d >> eb) & 1u);
        extra = d & ((1u << eb) - 1u);
    }
}
// RFC 1951 3.2.6: the fixed literal/length code of sym = 0 .. 287 and its bits (every fixed distance code is its symbol in 5)
BV_DEF_FN uint32_t bv_def_fixed_len(uint32_t sym) { return sym < 144u ? 8u : sym < 256u ? 9u : sym < 280u ? 7u : 8u; }
BV_DEF_FN uint32_t bv_def_fixed_code(uint32_t sym) { return sym < 144u ? 0x30u + sym : sym < 256u ? 0x190u + (sym - 144u) : sym < 280u ? sym - 256u : 0xc0u + (sym - 280u); }

BV_DEF_FN void bv_def_lensym(BvDefBits &b, uint32_t sym, uint32_t lane) {  // a literal, the end code or a length symbol in the fixed code
    const uint32_t l = bv_def_fixed_len(sym);
    bv_def_put(b, bv_def_rev(bv_def_fixed_code(sym), l), l, lane);
}
BV_DEF_FN void bv_def_match(BvDefBits &b, uint32_t len, uint32_t dist, uint32_t lane) {
    uint32_t sym, eb, extra;
    bv_def_len_sym(len - 3u, sym, eb, extra);
    const uint32_t l = bv_def_fixed_len(sym);  // (a code and its extra bits: at most 13 + 18 bits)
    bv_def_put(b, bv_def_rev(bv_def_fixed_code(sym), l) | (extra << l), l + eb, lane);
    bv_def_dist_sym(dist - 1u, sym, eb, extra);
    bv_def_put(b, bv_def_rev(sym, 5) | (extra << 5), 5u + eb, lane);
}

// text[0 .. n) as one final block with the fixed codes, from out + 18 on.  Returns the payload's bytes, or 0 when they would
// not be fewer than `stored_len`, the stored form's (nothing behind out + 16 + 2 + stored_len is written either way).
BV_DEF_FN uint32_t bv_def_fixed(const uint8_t *text, uint32_t n, uint8_t *out, uint32_t stored_len, BvDefState *S, uint32_t lane, uint32_t nlanes) {
    bv_def_clear(S, lane, nlanes);
    BvDefBits b;
    b.out = out + 16; b.pos = 0; b.limit = 2u + stored_len; b.cnt = 16u; b.over = 0; b.buf = 0;
    bv_def_put(b, 3u, 3, lane);  // BFINAL = 1, BTYPE = 01
    uint32_t cur = 0;            // the parse: the next position to code
    for (uint32_t base = 0; base < n && !b.over; base += BV_DEF_CHUNK) {
        bv_def_chunk(text, n, base, cur, S, lane, nlanes);
        const uint32_t end = base + BV_DEF_CHUNK < n ? base + BV_DEF_CHUNK : n;
        while (cur < end && !b.over) {
            const uint32_t i = cur - base, len = S->len[i];
            if (len) {
                bv_def_match(b, len, (uint32_t)S->dist[i] + 1u, lane);
                cur += len;
            } else {
                bv_def_lensym(b, text[cur], lane);
                cur += 1u;
            }
        }
        BV_DEF_WAVE_SYNC();
    }
    bv_def_lensym(b, 256u, lane);
    const uint32_t bytes = b.pos + (b.cnt + 7u) / 8u;  // from out + 16
    if (b.over || bytes > b.limit || bytes - 2u >= stored_len) return 0;
    if (lane == 0)
        for (uint32_t k = 0; k * 8u < b.cnt; ++k) out[16u + b.pos + k] = (uint8_t)(b.buf >> (8u * k));
    return bytes - 2u;
}

// The frame of one BGZF member around a payload of `plen` bytes that lies at out + 18; plen == 0: the stored form is chosen,
// and is written here.  crc_tab: bv_inf_crc_tables.  `crc_reduce` combines the lanes' CRC shares: on the device the xor over the
// wave, on the host (one lane, which has computed every share) the identity.  Returns the member's bytes.
template <class Reduce>
BV_DEF_FN uint32_t bv_def_frame(const uint8_t *text, uint32_t n, uint8_t *out, uint32_t plen, const uint32_t *crc_tab, uint32_t lane, uint32_t nlanes,
                                Reduce crc_reduce) {
    uint32_t share = 0;
    for (uint32_t s = lane; s < 64u; s += nlanes) share ^= bv_inf_crc_share(text, n, s, crc_tab);
    const uint32_t crc = ~crc_reduce(share);
    if (plen == 0) {
        plen = 5u + n;
        if (lane == 0) {
            out[18] = 1;  // BFINAL = 1, BTYPE = 00
            out[19] = (uint8_t)n; out[20] = (uint8_t)(n >> 8);
            out[21] = (uint8_t)~n; out[22] = (uint8_t)(~n >> 8);
        }
        for (uint32_t i = lane; i < n; i += nlanes) out[23u + i] = text[i];
    }
    const uint32_t total = 18u + plen + 8u;
    if (lane == 0) {
        const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        for (uint32_t k = 0; k < 16u; ++k) out[k] = head[k];
        out[16] = (uint8_t)(total - 1u); out[17] = (uint8_t)((total - 1u) >> 8);
        uint8_t *t = out + 18u + plen;
        for (uint32_t k = 0; k < 4u; ++k) { t[k] = (uint8_t)(crc >> (8u * k)); t[4u + k] = (uint8_t)(n >> (8u * k)); }
    }
    return total;
}

// One whole BGZF member of text[0 .. n), 1 <= n <= BV_DEF_MAX_BLOCK, at `out` (room for n + BV_DEF_MEMBER_EXTRA bytes; 4-byte
// aligned on the device).  crc_tab, crc_reduce: as bv_def_frame takes them.  Returns the member's bytes.
template <class Reduce>
BV_DEF_FN uint32_t bv_def_member(const uint8_t *text, uint32_t n, uint8_t *out, BvDefState *S, const uint32_t *crc_tab, uint32_t lane,
                                 uint32_t nlanes, Reduce crc_reduce) {
    const uint32_t plen = bv_def_fixed(text, n, out, 5u + n, S, lane, nlanes);
    return bv_def_frame(text, n, out, plen, crc_tab, lane, nlanes, crc_reduce);
}

#endif  // BV_DEFLATE_CORE_H
