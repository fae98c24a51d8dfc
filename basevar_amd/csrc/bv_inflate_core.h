// bv_inflate_core.h -- the DEFLATE (RFC 1951) decoder behind bv_engine_bgzf_inflate (include/basevar_amd_bgzf.h), as inline
// functions that the device kernel (bv_inflate.hip) and a plain g++ harness (tests/cpp/inflate_core_check.cpp, run under
// ASan + UBSan against zlib) both compile.  Nothing here allocates, and every access is bounded by the member itself:
//   reads of compressed input   by the payload length (bits behind it read as zero and are counted: BvInfBits::overrun),
//   writes of inflated bytes    by the member's ISIZE,
//   match sources               by the bytes already written in this member,
//   every loop                  by one of those, or by the fixed sizes of a block header.
//
// One wave decodes one member.  The code is written for `nlanes` lanes that all execute it with identical values (the bit
// buffer, the decoded symbols and every branch are the same in all lanes; a table read is a broadcast) and that share the
// work that is wide: clearing and filling the decode tables, copying matches and stored blocks.  `lane` only ever selects
// which of those bytes a lane writes.  On the CPU the same code runs with lane 0 of 1.  The tables and the output window live
// in LDS on the device; the operations of one wave on LDS execute in order, so a lane may read what another lane of the same
// wave wrote in an earlier instruction -- BV_INF_WAVE_SYNC() only keeps the compiler from reordering across it.
//
// What is accepted is what zlib accepts (inflate.c / inftrees.c of zlib 1.2.11), and a damaged stream is named as zlib, asked
// to inflate into exactly ISIZE bytes, would leave it: a data error -> BV_BGZF_BAD_DEFLATE; input exhausted, output full
// before the final block ended or short at its end -> BV_BGZF_BAD_SIZE.
#ifndef BV_INFLATE_CORE_H
#define BV_INFLATE_CORE_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BV_INF_FN __host__ __device__ inline
#else
#define BV_INF_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
// lanes of one wave hand bytes to each other through LDS: a release / acquire pair at wavefront scope (no instruction: the
// LDS operations of a wave execute in order) around the scheduling barrier, so the order does not rest on alias analysis
#define BV_INF_WAVE_SYNC()                                      \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)
#else
#define BV_INF_WAVE_SYNC() ((void)0)
#endif

// per-member status (mirrors include/basevar_amd_bgzf.h; bv_inflate.hip asserts that the two agree)
enum { BV_INF_OK = 0, BV_INF_BAD_HEADER = 1, BV_INF_BAD_DEFLATE = 2, BV_INF_BAD_SIZE = 3, BV_INF_BAD_CRC = 4 };

#define BV_INF_MAX_ISIZE 65536u    // a BGZF member inflates to at most 64 KiB
#define BV_INF_MIN_MEMBER 26u      // 12 header bytes + the 6-byte BC subfield + CRC32 + ISIZE (and an empty payload)
#define BV_INF_LIT_BITS 11u        // primary table of the literal/length code; longer codes take the canonical walk
#define BV_INF_DIST_BITS 10u
#define BV_INF_CL_BITS 7u          // the code-length code: at most 7 bits, so its table (in `dist`) is complete

// Decode state of one member: ~7.5 KiB (LDS on the device).
struct BvInfTables {
    uint16_t lit[1u << BV_INF_LIT_BITS];    // (symbol << 4) | code length; 0: not a code of at most BV_INF_LIT_BITS bits
    uint16_t dist[1u << BV_INF_DIST_BITS];  // the same for distances (and, while a header is read, for the code-length code)
    uint16_t litsym[288], distsym[32];      // symbols in canonical order (by length, then by value)
    uint16_t litcnt[16], distcnt[16];       // codes per length
    uint16_t offs[16];                      // scratch of the table build
    uint8_t lens[352];                      // the 19 lengths of the code-length code, then HLIT + HDIST <= 286 + 30 code lengths
    uint32_t block_mask;                    // bit t: a block of type t was met (what the tests' corpus check reads)
};

struct BvInfBits {
    const uint8_t *in;
    uint32_t n;     // payload bytes
    uint32_t pos;   // bytes taken into `buf` (beyond n: zero bytes that do not exist)
    uint32_t cnt;   // valid bits in buf
    uint64_t buf;
};

// at least 33 bits in the buffer afterwards
BV_INF_FN void bv_inf_refill(BvInfBits &b) {
    if (b.cnt > 32u) return;
    uint32_t w = 0;
    if (b.pos + 4u <= b.n) {
        memcpy(&w, b.in + b.pos, 4);
    } else {
        for (uint32_t k = 0; k < 4u; ++k)
            if (b.pos + k < b.n) w |= (uint32_t)b.in[b.pos + k] << (8u * k);
    }
    b.buf |= (uint64_t)w << b.cnt;
    b.cnt += 32u;
    b.pos += 4u;
}
BV_INF_FN uint32_t bv_inf_peek(const BvInfBits &b, uint32_t k) { return (uint32_t)b.buf & ((1u << k) - 1u); }
BV_INF_FN void bv_inf_drop(BvInfBits &b, uint32_t k) { b.buf >>= k; b.cnt -= k; }
BV_INF_FN uint32_t bv_inf_take(BvInfBits &b, uint32_t k) { const uint32_t v = bv_inf_peek(b, k); bv_inf_drop(b, k); return v; }
// more bits consumed than the payload holds: the stream is truncated (zlib would be waiting for input)
BV_INF_FN bool bv_inf_overrun(const BvInfBits &b) { return (uint64_t)b.pos * 8u - b.cnt > (uint64_t)b.n * 8u; }

BV_INF_FN uint32_t bv_inf_rev16(uint32_t v) {
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    return ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
}

enum { BV_INF_CODES = 0, BV_INF_LENS = 1, BV_INF_DISTS = 2 };

// Build the decoder of one code from lens[0 .. n): zlib's acceptance rule (inftrees.c) first -- never over-subscribed;
// incomplete only when the longest code is one bit, and never for the code-length code; a set without any code is let through
// (every decode then fails) -- and nothing is written to `tab` for a refused set.  Returns 0, or -1 for a refused set.
BV_INF_FN int bv_inf_build(const uint8_t *lens, uint32_t n, int type, uint16_t *tab, uint32_t tab_bits, uint16_t *cnt, uint16_t *sym,
                           uint16_t *offs, uint32_t lane, uint32_t nlanes) {
    for (uint32_t l = 0; l < 16u; ++l) cnt[l] = 0;
    BV_INF_WAVE_SYNC();
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = lens[i] & 15u;
        cnt[l] = (uint16_t)(cnt[l] + 1u);
        BV_INF_WAVE_SYNC();
    }
    uint32_t max = 15;
    while (max > 0 && cnt[max] == 0) --max;
    int32_t left = 1;
    for (uint32_t l = 1; l < 16u; ++l) {
        left = left * 2 - (int32_t)cnt[l];
        if (left < 0) return -1;
    }
    if (left > 0 && max != 0 && (type == BV_INF_CODES || max != 1)) return -1;
    uint32_t o = 0;
    for (uint32_t l = 1; l < 16u; ++l) {
        offs[l] = (uint16_t)o;
        o += cnt[l];
    }
    BV_INF_WAVE_SYNC();
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = lens[i] & 15u;
        if (l) {
            const uint32_t k = offs[l];  // < number of coded symbols <= n
            sym[k] = (uint16_t)i;
            offs[l] = (uint16_t)(k + 1u);
            BV_INF_WAVE_SYNC();
        }
    }
    const uint32_t size = 1u << tab_bits;
    for (uint32_t j = lane; j < size; j += nlanes) tab[j] = 0;
    BV_INF_WAVE_SYNC();
    // canonical codes in order; code k of length l fills every entry whose low l bits are the code, bit-reversed
    uint32_t code = 0, prev = 0;
    for (uint32_t k = 0; k < o; ++k) {
        const uint32_t s = sym[k], l = lens[s] & 15u;
        code <<= (l - prev);
        prev = l;
        if (l > tab_bits) break;
        const uint32_t rev = bv_inf_rev16(code) >> (16u - l);
        const uint16_t e = (uint16_t)((s << 4) | l);
        for (uint32_t j = rev + (lane << l); j < size; j += nlanes << l) tab[j] = e;
        ++code;
    }
    BV_INF_WAVE_SYNC();
    return 0;
}

// One symbol, or -1 where the next bits are no code (an incomplete or an empty set); zlib takes one bit for those.
// Needs 15 bits in the buffer.
BV_INF_FN int32_t bv_inf_decode(BvInfBits &b, const uint16_t *tab, uint32_t tab_bits, const uint16_t *cnt, const uint16_t *sym) {
    const uint32_t e = tab[bv_inf_peek(b, tab_bits)];
    if (e) {
        bv_inf_drop(b, e & 15u);
        return (int32_t)(e >> 4);
    }
    int32_t code = 0, first = 0, index = 0;
    uint32_t bits = (uint32_t)b.buf;
    for (uint32_t l = 1; l < 16u; ++l) {
        code |= (int32_t)(bits & 1u);
        bits >>= 1;
        const int32_t c = cnt[l];
        if (code - c < first) {
            bv_inf_drop(b, l);
            return sym[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    bv_inf_drop(b, 1);
    return -1;
}

// Inflate one raw DEFLATE stream of `in_len` bytes into out[0 .. isize).  Returns BV_INF_OK (exactly isize bytes written and
// the final block ended), BV_INF_BAD_DEFLATE or BV_INF_BAD_SIZE.  Payload bytes behind the final block are ignored.
BV_INF_FN int bv_inf_stream(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t isize, BvInfTables *T, uint32_t lane,
                            uint32_t nlanes) {
#define BV_INF_DATA_ERROR() return bv_inf_overrun(b) ? BV_INF_BAD_SIZE : BV_INF_BAD_DEFLATE
    BvInfBits b;
    b.in = in; b.n = in_len; b.pos = 0; b.cnt = 0; b.buf = 0;
    uint32_t op = 0;  // bytes written, <= isize
    if (lane == 0) T->block_mask = 0;
    for (;;) {
        bv_inf_refill(b);
        const uint32_t bfinal = bv_inf_take(b, 1), btype = bv_inf_take(b, 2);
        if (bv_inf_overrun(b)) return BV_INF_BAD_SIZE;
        if (btype == 3u) return BV_INF_BAD_DEFLATE;
        if (lane == 0) T->block_mask |= 1u << btype;
        if (btype == 0u) {
            bv_inf_drop(b, b.cnt & 7u);
            bv_inf_refill(b);
            const uint32_t len = bv_inf_take(b, 16), nlen = bv_inf_take(b, 16);
            if (bv_inf_overrun(b)) return BV_INF_BAD_SIZE;
            if (len != (nlen ^ 0xffffu)) return BV_INF_BAD_DEFLATE;
            const uint32_t at = b.pos - b.cnt / 8u;  // <= in_len: nothing beyond the payload has been consumed
            uint32_t c = len;
            if (c > in_len - at) c = in_len - at;
            if (c > isize - op) c = isize - op;
            for (uint32_t i = lane; i < c; i += nlanes) out[op + i] = in[at + i];
            BV_INF_WAVE_SYNC();
            op += c;
            if (c < len) return BV_INF_BAD_SIZE;  // input exhausted or output full inside the block
            b.pos = at + len; b.cnt = 0; b.buf = 0;
        } else {
            if (btype == 1u) {
                for (uint32_t i = lane; i < 320u; i += nlanes) T->lens[i] = i < 144u ? 8 : i < 256u ? 9 : i < 280u ? 7 : i < 288u ? 8 : 5;
                BV_INF_WAVE_SYNC();
                // (complete sets: the build cannot refuse them)
                bv_inf_build(T->lens, 288, BV_INF_LENS, T->lit, BV_INF_LIT_BITS, T->litcnt, T->litsym, T->offs, lane, nlanes);
                bv_inf_build(T->lens + 288, 32, BV_INF_DISTS, T->dist, BV_INF_DIST_BITS, T->distcnt, T->distsym, T->offs, lane, nlanes);
            } else {
                bv_inf_refill(b);
                const uint32_t nl = bv_inf_take(b, 5) + 257u, nd = bv_inf_take(b, 5) + 1u, nc = bv_inf_take(b, 4) + 4u;
                if (bv_inf_overrun(b)) return BV_INF_BAD_SIZE;
                if (nl > 286u || nd > 30u) return BV_INF_BAD_DEFLATE;
                for (uint32_t i = lane; i < 19u; i += nlanes) T->lens[i] = 0;
                BV_INF_WAVE_SYNC();
                for (uint32_t i = 0; i < nc; ++i) {
                    bv_inf_refill(b);
                    const uint32_t v = bv_inf_take(b, 3);
                    // the order of RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                    const uint32_t at = i < 3u ? 16u + i : i == 3u ? 0u : (i & 1u) ? (19u - i) / 2u : 6u + i / 2u;
                    if (lane == 0) T->lens[at] = (uint8_t)v;
                }
                BV_INF_WAVE_SYNC();
                if (bv_inf_overrun(b)) return BV_INF_BAD_SIZE;
                if (bv_inf_build(T->lens, 19, BV_INF_CODES, T->dist, BV_INF_CL_BITS, T->distcnt, T->distsym, T->offs, lane, nlanes))
                    BV_INF_DATA_ERROR();
                // the code lengths sit behind the 19 of the code-length code while they are read
                uint8_t *cl = T->lens + 19;
                const uint32_t total = nl + nd;  // <= 316
                uint32_t i = 0;
                while (i < total) {
                    bv_inf_refill(b);
                    int32_t s = bv_inf_decode(b, T->dist, BV_INF_CL_BITS, T->distcnt, T->distsym);
                    if (s < 0) s = 0;  // a code-length code without any code: zlib reads each length as 0, one bit apiece
                    uint32_t rep = 1, val = (uint32_t)s;
                    if (s == 16) {
                        if (i == 0) BV_INF_DATA_ERROR();
                        val = cl[i - 1];
                        rep = 3u + bv_inf_take(b, 2);
                    } else if (s == 17) {
                        val = 0;
                        rep = 3u + bv_inf_take(b, 3);
                    } else if (s == 18) {
                        val = 0;
                        rep = 11u + bv_inf_take(b, 7);
                    }
                    if (bv_inf_overrun(b)) return BV_INF_BAD_SIZE;
                    if (i + rep > total) return BV_INF_BAD_DEFLATE;
                    if (lane == 0)
                        for (uint32_t k = 0; k < rep; ++k) cl[i + k] = (uint8_t)val;
                    BV_INF_WAVE_SYNC();
                    i += rep;
                }
                if (cl[256] == 0) return BV_INF_BAD_DEFLATE;  // a block that can end has a code for symbol 256
                if (bv_inf_build(cl, nl, BV_INF_LENS, T->lit, BV_INF_LIT_BITS, T->litcnt, T->litsym, T->offs, lane, nlanes))
                    return BV_INF_BAD_DEFLATE;
                if (bv_inf_build(cl + nl, nd, BV_INF_DISTS, T->dist, BV_INF_DIST_BITS, T->distcnt, T->distsym, T->offs, lane, nlanes))
                    return BV_INF_BAD_DEFLATE;
            }
            for (;;) {
                bv_inf_refill(b);
                const int32_t s = bv_inf_decode(b, T->lit, BV_INF_LIT_BITS, T->litcnt, T->litsym);
                if (bv_inf_overrun(b)) return BV_INF_BAD_SIZE;
                if (s < 0 || s > 285) return BV_INF_BAD_DEFLATE;
                if (s < 256) {
                    if (op == isize) return BV_INF_BAD_SIZE;
                    if (lane == 0) out[op] = (uint8_t)s;
                    BV_INF_WAVE_SYNC();
                    ++op;
                    continue;
                }
                if (s == 256) break;
                uint32_t len;
                if (s < 265) {
                    len = (uint32_t)s - 254u;
                } else if (s == 285) {
                    len = 258;
                } else {
                    const uint32_t e = ((uint32_t)s - 261u) >> 2;
                    len = 3u + ((4u + (((uint32_t)s - 261u) & 3u)) << e) + bv_inf_take(b, e);
                }
                bv_inf_refill(b);
                const int32_t d = bv_inf_decode(b, T->dist, BV_INF_DIST_BITS, T->distcnt, T->distsym);
                if (d < 0 || d > 29) BV_INF_DATA_ERROR();
                uint32_t dist;
                if (d < 4) {
                    dist = (uint32_t)d + 1u;
                } else {
                    const uint32_t e = ((uint32_t)d >> 1) - 1u;
                    dist = 1u + ((2u + ((uint32_t)d & 1u)) << e) + bv_inf_take(b, e);
                }
                if (bv_inf_overrun(b)) return BV_INF_BAD_SIZE;
                if (op == isize) return BV_INF_BAD_SIZE;
                if (dist > op) return BV_INF_BAD_DEFLATE;  // a match source before the first byte of this member
                uint32_t c = len;
                if (c > isize - op) c = isize - op;
                const uint32_t from = op - dist;
                if (dist >= c) {
                    for (uint32_t i = lane; i < c; i += nlanes) out[op + i] = out[from + i];
                } else if (dist == 1u) {
                    const uint8_t v = out[from];
                    for (uint32_t i = lane; i < c; i += nlanes) out[op + i] = v;
                } else {  // the match overlaps its own output: byte i repeats byte i mod dist of what was there before
                    for (uint32_t i = lane; i < c; i += nlanes) out[op + i] = out[from + i % dist];
                }
                BV_INF_WAVE_SYNC();
                op += c;
                if (c < len) return BV_INF_BAD_SIZE;
            }
        }
        if (bfinal) break;
    }
    if (bv_inf_overrun(b)) return BV_INF_BAD_SIZE;
    return op == isize ? BV_INF_OK : BV_INF_BAD_SIZE;
#undef BV_INF_DATA_ERROR
}

// ---- CRC32 (the gzip polynomial, reflected): slicing-by-4 tables, per-lane slices of BV_INF_CRC_SLICE bytes, and the GF(2)
// shift that moves a slice's remainder to its place in the member.
#define BV_INF_CRC_POLY 0xedb88320u
#define BV_INF_CRC_SLICE 1024u  // 64 lanes x 1 KiB = the largest member

// tab[4][256]; the caller orders the fill before the first use (BV_INF_WAVE_SYNC is inside)
BV_INF_FN void bv_inf_crc_tables(uint32_t *tab, uint32_t lane, uint32_t nlanes) {
    for (uint32_t i = lane; i < 256u; i += nlanes) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? BV_INF_CRC_POLY ^ (c >> 1) : c >> 1;
        tab[i] = c;
    }
    BV_INF_WAVE_SYNC();
    for (uint32_t t = 1; t < 4u; ++t) {
        for (uint32_t i = lane; i < 256u; i += nlanes) {
            const uint32_t c = tab[(t - 1u) * 256u + i];
            tab[t * 256u + i] = (c >> 8) ^ tab[c & 0xffu];
        }
        BV_INF_WAVE_SYNC();
    }
}

// a(x) * b(x) mod P(x), reflected bit order (zlib's multmodp)
BV_INF_FN uint32_t bv_inf_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ BV_INF_CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) mod P
BV_INF_FN uint32_t bv_inf_xpow8(uint32_t n) {
    uint32_t p = 0x80000000u, q = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1u) p = bv_inf_mulmod(q, p);
        q = bv_inf_mulmod(q, q);
    }
    return p;
}

// Lane `slice`'s share of the CRC32 of win[0 .. n): the xor of the shares of slices 0 .. 63, inverted, is the CRC32.
// `win` is 4-byte aligned on the device (the LDS window); any alignment on the host.
BV_INF_FN uint32_t bv_inf_crc_share(const uint8_t *win, uint32_t n, uint32_t slice, const uint32_t *tab) {
    const uint32_t lo = slice * BV_INF_CRC_SLICE < n ? slice * BV_INF_CRC_SLICE : n;
    const uint32_t hi = lo + BV_INF_CRC_SLICE < n ? lo + BV_INF_CRC_SLICE : n;
    uint32_t c = 0, i = lo;
    for (; i + 4u <= hi; i += 4u) {
        uint32_t w;
#if defined(__HIP_DEVICE_COMPILE__)
        w = *reinterpret_cast<const uint32_t *>(win + i);
#else
        memcpy(&w, win + i, 4);
#endif
        c ^= w;
        c = tab[768u + (c & 0xffu)] ^ tab[512u + ((c >> 8) & 0xffu)] ^ tab[256u + ((c >> 16) & 0xffu)] ^ tab[c >> 24];
    }
    for (; i < hi; ++i) c = tab[(c ^ win[i]) & 0xffu] ^ (c >> 8);
    uint32_t share = hi > lo ? bv_inf_mulmod(bv_inf_xpow8(n - hi), c) : 0u;
    if (slice == 0) share ^= bv_inf_mulmod(bv_inf_xpow8(n), 0xffffffffu);  // what the initial value becomes behind n bytes
    return share;
}

// ---- the BGZF wrapper of one member (SAM specification 4.1): a gzip member with FLG = FEXTRA whose extra field carries the
// 'B' 'C' subfield with the member's length - 1, then the payload, then CRC32 and ISIZE.
struct BvBgzfMember {
    uint32_t payload_off, payload_len, crc, isize;
};
BV_INF_FN uint32_t bv_inf_le32(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
// BV_INF_OK or BV_INF_BAD_HEADER (a length in the BC field that is not the packing's is a bad header)
BV_INF_FN int bv_bgzf_member_parse(const uint8_t *m, uint64_t mlen, BvBgzfMember *o) {
    o->payload_off = o->payload_len = o->crc = o->isize = 0;
    if (mlen < BV_INF_MIN_MEMBER || mlen > 65536u) return BV_INF_BAD_HEADER;
    if (m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || m[3] != 4) return BV_INF_BAD_HEADER;
    const uint32_t xlen = m[10] | ((uint32_t)m[11] << 8);
    if (12u + xlen + 8u > mlen) return BV_INF_BAD_HEADER;
    uint32_t found = 0, bsize = 0;
    for (uint32_t at = 12; at + 4u <= 12u + xlen;) {
        const uint32_t slen = m[at + 2] | ((uint32_t)m[at + 3] << 8);
        if (at + 4u + slen > 12u + xlen) return BV_INF_BAD_HEADER;
        if (m[at] == 'B' && m[at + 1] == 'C') {
            if (slen != 2u) return BV_INF_BAD_HEADER;
            bsize = m[at + 4] | ((uint32_t)m[at + 5] << 8);
            ++found;
        }
        at += 4u + slen;
    }
    if (found != 1u || bsize + 1u != mlen) return BV_INF_BAD_HEADER;
    o->payload_off = 12u + xlen;
    o->payload_len = (uint32_t)mlen - o->payload_off - 8u;
    o->crc = bv_inf_le32(m + mlen - 8);
    o->isize = bv_inf_le32(m + mlen - 4);
    return BV_INF_OK;
}

#endif  // BV_INFLATE_CORE_H
