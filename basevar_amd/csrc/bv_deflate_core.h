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
#define BV_DEF_NO_HASH 0xffffffffu
#define BV_DEF_TEXT_PAD 8u         // bytes behind the text that the device's window must own (bv_def_load4 reads whole words)

// Match state of one block: 8 KiB of table + 0.7 KiB (LDS on the device).
struct BvDefState {
    uint16_t head[1u << BV_DEF_HASH_BITS];  // position + 1 of the latest position with this hash; 0: none
    uint32_t hash[BV_DEF_CHUNK];            // the chunk's hashes (BV_DEF_NO_HASH: fewer than 4 bytes left)
    uint16_t cand[BV_DEF_CHUNK];            // position + 1 of the candidate; 0: none
    uint16_t len[BV_DEF_CHUNK];             // match length, 0: a literal
    uint16_t dist[BV_DEF_CHUNK];
    uint8_t last[BV_DEF_CHUNK];             // no later position of the chunk has this hash
};

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
        if (b.pos + 4u > b.limit) {
            b.over = 1u;
        } else if (lane == 0) {
            const uint32_t w = (uint32_t)b.buf;
#if defined(__HIP_DEVICE_COMPILE__)
            *reinterpret_cast<uint32_t *>(b.out + b.pos) = w;
#else
            memcpy(b.out + b.pos, &w, 4);
#endif
        }
        b.pos += 4u;
        b.buf >>= 32;
        b.cnt -= 32u;
    }
}
// an n-bit Huffman code, which DEFLATE packs from its most significant bit
BV_DEF_FN uint32_t bv_def_rev(uint32_t code, uint32_t n) { return bv_inf_rev16(code) >> (16u - n); }

BV_DEF_FN void bv_def_literal(BvDefBits &b, uint32_t v, uint32_t lane) {
    if (v < 144u) bv_def_put(b, bv_def_rev(0x30u + v, 8), 8, lane);
    else bv_def_put(b, bv_def_rev(0x190u + (v - 144u), 9), 9, lane);
}
BV_DEF_FN void bv_def_lensym(BvDefBits &b, uint32_t sym, uint32_t lane) {  // 256 .. 287 of the fixed literal/length code
    if (sym < 280u) bv_def_put(b, bv_def_rev(sym - 256u, 7), 7, lane);
    else bv_def_put(b, bv_def_rev(0xc0u + (sym - 280u), 8), 8, lane);
}
BV_DEF_FN void bv_def_match(BvDefBits &b, uint32_t len, uint32_t dist, uint32_t lane) {
    const uint32_t l = len - 3u;
    if (len == 258u) {
        bv_def_lensym(b, 285u, lane);
    } else if (l < 8u) {
        bv_def_lensym(b, 257u + l, lane);
    } else {
        const uint32_t eb = (31u - (uint32_t)__builtin_clz(l)) - 2u;
        bv_def_lensym(b, 261u + 4u * eb + ((l >> eb) & 3u), lane);
        bv_def_put(b, l & ((1u << eb) - 1u), eb, lane);
    }
    const uint32_t d = dist - 1u;
    if (d < 4u) {
        bv_def_put(b, bv_def_rev(d, 5), 5, lane);
    } else {
        const uint32_t eb = (31u - (uint32_t)__builtin_clz(d)) - 1u;
        bv_def_put(b, bv_def_rev(2u * eb + 2u + ((d >> eb) & 1u), 5), 5, lane);
        bv_def_put(b, d & ((1u << eb) - 1u), eb, lane);
    }
}

// text[0 .. n) as one final block with the fixed codes, from out + 18 on.  Returns the payload's bytes, or 0 when they would
// not be fewer than `stored_len`, the stored form's (nothing behind out + 16 + 2 + stored_len is written either way).
BV_DEF_FN uint32_t bv_def_fixed(const uint8_t *text, uint32_t n, uint8_t *out, uint32_t stored_len, BvDefState *S, uint32_t lane, uint32_t nlanes) {
    for (uint32_t i = lane; i < (1u << BV_DEF_HASH_BITS); i += nlanes) S->head[i] = 0;
    BV_DEF_WAVE_SYNC();
    BvDefBits b;
    b.out = out + 16; b.pos = 0; b.limit = 2u + stored_len; b.cnt = 16u; b.over = 0; b.buf = 0;
    bv_def_put(b, 3u, 3, lane);  // BFINAL = 1, BTYPE = 01
    uint32_t cur = 0;            // the parse: the next position to code
    for (uint32_t base = 0; base < n && !b.over; base += BV_DEF_CHUNK) {
        const bool measure = cur < base + BV_DEF_CHUNK;  // else an earlier match covers the whole chunk: only the table is kept
        for (uint32_t i = lane; i < BV_DEF_CHUNK; i += nlanes) {
            const uint32_t p = base + i;
            uint32_t h = BV_DEF_NO_HASH, c = 0;
            if (p + BV_DEF_MIN_MATCH <= n) {
                h = bv_def_hash(bv_def_load4(text, p));
                c = S->head[h];
            }
            S->hash[i] = h;
            S->cand[i] = (uint16_t)c;
        }
        BV_DEF_WAVE_SYNC();
        for (uint32_t i = lane; i < BV_DEF_CHUNK; i += nlanes) {
            const uint32_t p = base + i, h = S->hash[i];
            uint32_t c = S->cand[i], last = 1u, len = 0;
            if (h != BV_DEF_NO_HASH) {
                for (uint32_t j = 0; j < BV_DEF_CHUNK; ++j) {
                    const bool same = S->hash[j] == h;
                    if (same && j < i) c = base + j + 1u;
                    if (same && j > i) last = 0u;
                }
            }
            if (measure && c != 0 && p >= cur && p - (c - 1u) <= BV_DEF_WINDOW) {
                const uint32_t q = c - 1u, maxl = n - p < BV_DEF_MAX_MATCH ? n - p : BV_DEF_MAX_MATCH;
                while (len + 4u <= maxl && bv_def_load4(text, p + len) == bv_def_load4(text, q + len)) len += 4u;
                while (len < maxl && text[p + len] == text[q + len]) ++len;
                if (len < BV_DEF_MIN_MATCH) len = 0;
            }
            S->last[i] = (uint8_t)last;
            S->len[i] = (uint16_t)len;
            S->dist[i] = (uint16_t)(len ? p - (c - 1u) - 1u : 0u);  // distance - 1: 0 .. 32767
        }
        BV_DEF_WAVE_SYNC();
        for (uint32_t i = lane; i < BV_DEF_CHUNK; i += nlanes)
            if (S->hash[i] != BV_DEF_NO_HASH && S->last[i]) S->head[S->hash[i]] = (uint16_t)(base + i + 1u);
        const uint32_t end = base + BV_DEF_CHUNK < n ? base + BV_DEF_CHUNK : n;
        while (cur < end && !b.over) {
            const uint32_t i = cur - base, len = S->len[i];
            if (len) {
                bv_def_match(b, len, (uint32_t)S->dist[i] + 1u, lane);
                cur += len;
            } else {
                bv_def_literal(b, text[cur], lane);
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

// One whole BGZF member of text[0 .. n), 1 <= n <= BV_DEF_MAX_BLOCK, at `out` (room for n + BV_DEF_MEMBER_EXTRA bytes; 4-byte
// aligned on the device).  crc_tab: bv_inf_crc_tables.  `crc_reduce` combines the lanes' CRC shares: on the device the xor
// over the wave, on the host (one lane, which has computed every share) the identity.  Returns the member's bytes.
template <class Reduce>
BV_DEF_FN uint32_t bv_def_member(const uint8_t *text, uint32_t n, uint8_t *out, BvDefState *S, const uint32_t *crc_tab, uint32_t lane,
                                 uint32_t nlanes, Reduce crc_reduce) {
    uint32_t share = 0;
    for (uint32_t s = lane; s < 64u; s += nlanes) share ^= bv_inf_crc_share(text, n, s, crc_tab);
    const uint32_t crc = ~crc_reduce(share);
    const uint32_t stored_len = 5u + n;
    uint32_t plen = bv_def_fixed(text, n, out, stored_len, S, lane, nlanes);
    if (plen == 0) {
        plen = stored_len;
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

#endif  // BV_DEFLATE_CORE_H
