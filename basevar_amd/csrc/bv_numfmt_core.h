// bv_numfmt_core.h -- the decimal text of the numbers a VCF head and a CVG row print (bv_record_text_core.h), as inline
// functions that the device kernels (bv_record_text.hip) and a plain g++ harness (tests/cpp/record_text_check.cpp) both
// compile, as bv_vcf_core.h is.  No printf, no floating-point arithmetic: a double is taken apart into its bits and the
// digits come from integer arithmetic of at most 128 bits (multiplies, shifts and compares; no 128-bit division).
//
// THE TEXT, defined without reference to lanes.  A finite double is v = (-1)^sign * k / 2^s with integers k < 2^53 and s
// (k = the fraction with its hidden bit and s = 1075 - the biased exponent; k = the fraction and s = 1074 for a denormal).
// rhe(x) is x rounded to an integer, a tie to the even one.
//
//   f6(v)  = "%f" of v, what std::to_string(double) gives (QUAL, QD, FS, SOR), for finite |v| < 2^63:
//            q = rhe(k * 10^6 / 2^s); the text is '-' if the sign bit is set (so "-0.000000" for -0.0 and for tiny negatives),
//            the decimal of q / 10^6 (at least one digit), '.', and the six digits of q mod 10^6.
//            For s <= 0 q is k * 2^-s * 10^6 exactly; for s > 74 it is 0 (k * 10^6 < 2^73 is below half of 2^s).
//            Computed as the integer part k >> s and rhe(f * 10^6 / 2^s) of the fraction bits f = k mod 2^s, which is the
//            same q (10^6 is even, so the parities agree) with the carry of a fraction that rounds to 10^6.
//   g6(v)  = "%g" of v at six significant digits (CM_AF, CM_CAF, the group AFs), for v = +-0 and 2^-40 <= |v| < 999999.5:
//            +-0 is "0" / "-0".  Otherwise E is the integer with 10^E <= |v| < 10^(E+1), found by exact comparison of
//            k with 10^E * 2^s (E >= 0) or of k * 10^-E with 2^s (E < 0); n = rhe(k * 10^(5-E) / 2^s), 10^5 <= n <= 10^6,
//            and n == 10^6 becomes n = 10^5, E += 1.  With d0 .. d5 the digits of n and trailing zeros (and a point left
//            bare by them) dropped:   -4 <= E < 6:  the fixed notation of d0.d1d2d3d4d5 * 10^E
//                                     E < -4:       d0[.d1 ..]e-XX, XX = -E in two digits
//            (E >= 6 does not occur: |v| >= 999999.5 would print "1e+06" and is outside the domain.)
//   i32(u) = the decimal of (int)u for a uint32_t u, what std::to_string((int)u) gives: 0x80000000 is "-2147483648".
//   u32(u) = the decimal of u (POS).
//   iod(v) = the decimal of (int)v, truncation toward zero, for finite |v| < 2^31 (the three rank sums); "0" for -0.5.
// bv_numfmt_*_ok(v) says whether v lies in the domain; NaN, +-inf and everything beyond the bounds do not.
//
// A number is first reduced to a bv_numfmt_val, a few registers; bv_numfmt_len gives its bytes and bv_numfmt_put writes them.
// A value outside its domain becomes BV_NUM_BAD, of no bytes.
#ifndef BV_NUMFMT_CORE_H
#define BV_NUMFMT_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define BV_NUMFMT_FN __host__ __device__ inline
#else
#define BV_NUMFMT_FN inline
#endif

typedef unsigned __int128 bv_u128;

enum { BV_NUM_NONE = 0, BV_NUM_UINT = 1, BV_NUM_F6 = 2, BV_NUM_G6 = 3, BV_NUM_BAD = 4 };

typedef struct bv_numfmt_val {
    uint64_t a;    // UINT: the magnitude; F6: the integer part
    uint32_t b;    // F6: the six decimals as an integer; G6: n with its trailing zeros dropped
    int32_t e;     // G6: E
    uint8_t kind;  // BV_NUM_*
    uint8_t neg;   // a '-' in front
    uint8_t nd;    // G6: digits of b, 1 .. 6
} bv_numfmt_val;

#define BV_NUMFMT_BITS_2M40 0x3D70000000000000ull      /* 2^-40 */
#define BV_NUMFMT_BITS_999999_5 0x412E847F00000000ull  /* 999999.5 = 1999999 / 2 */

BV_NUMFMT_FN uint64_t bv_numfmt_bits(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}

// v = k / 2^s for a finite v
BV_NUMFMT_FN void bv_numfmt_split(uint64_t bits, uint64_t *k, int32_t *s) {
    const uint32_t eb = (uint32_t)(bits >> 52) & 0x7ffu;
    const uint64_t frac = bits & ((1ull << 52) - 1ull);
    *k = eb ? (frac | (1ull << 52)) : frac;
    *s = eb ? 1075 - (int32_t)eb : 1074;
}

BV_NUMFMT_FN bool bv_numfmt_f6_ok(double v) { return ((bv_numfmt_bits(v) >> 52) & 0x7ffu) < 1023u + 63u; }
BV_NUMFMT_FN bool bv_numfmt_g6_ok(double v) {
    const uint64_t a = bv_numfmt_bits(v) & ~(1ull << 63);  // of non-negative doubles the bits order as the values do
    return a == 0 || (a >= BV_NUMFMT_BITS_2M40 && a < BV_NUMFMT_BITS_999999_5);
}
BV_NUMFMT_FN bool bv_numfmt_iod_ok(double v) { return ((bv_numfmt_bits(v) >> 52) & 0x7ffu) < 1023u + 31u; }

BV_NUMFMT_FN uint64_t bv_numfmt_pow10(uint32_t e) {  // e <= 19
    uint64_t p = 1;
    for (uint32_t i = 0; i < e; ++i) p *= 10ull;
    return p;
}

BV_NUMFMT_FN uint32_t bv_numfmt_digits(uint64_t x) {
    uint32_t n = 1;
    while (x >= 10ull) { x /= 10ull; ++n; }
    return n;
}

// rhe(p / 2^s), 0 < s < 128, p < 2^127
BV_NUMFMT_FN uint64_t bv_numfmt_rhe_shift(bv_u128 p, uint32_t s) {
    const bv_u128 q = p >> s, rem = p - (q << s), half = (bv_u128)1 << (s - 1u);
    uint64_t r = (uint64_t)q;
    if (rem > half || (rem == half && (r & 1ull))) ++r;
    return r;
}

BV_NUMFMT_FN bv_numfmt_val bv_numfmt_none(void) {
    bv_numfmt_val o;
    o.a = 0; o.b = 0; o.e = 0; o.kind = BV_NUM_NONE; o.neg = 0; o.nd = 0;
    return o;
}
BV_NUMFMT_FN bv_numfmt_val bv_numfmt_bad(void) {
    bv_numfmt_val o = bv_numfmt_none();
    o.kind = BV_NUM_BAD;
    return o;
}
BV_NUMFMT_FN bv_numfmt_val bv_numfmt_u32(uint32_t u) {
    bv_numfmt_val o = bv_numfmt_none();
    o.kind = BV_NUM_UINT; o.a = u;
    return o;
}
BV_NUMFMT_FN bv_numfmt_val bv_numfmt_i32(uint32_t u) {
    bv_numfmt_val o = bv_numfmt_none();
    o.kind = BV_NUM_UINT;
    o.neg = (uint8_t)(u >> 31);
    o.a = o.neg ? (uint64_t)(0u - u) : (uint64_t)u;  // 0 - 0x80000000 is 0x80000000, the magnitude of INT_MIN
    return o;
}

BV_NUMFMT_FN bv_numfmt_val bv_numfmt_iod(double v) {
    if (!bv_numfmt_iod_ok(v)) return bv_numfmt_bad();
    const uint64_t bits = bv_numfmt_bits(v);
    uint64_t k; int32_t s;
    bv_numfmt_split(bits, &k, &s);
    bv_numfmt_val o = bv_numfmt_none();
    o.kind = BV_NUM_UINT;
    o.a = s >= 64 ? 0ull : s >= 0 ? k >> s : k << -s;  // |v| < 2^31: s >= 22
    o.neg = (uint8_t)((bits >> 63) && o.a != 0);
    return o;
}

BV_NUMFMT_FN bv_numfmt_val bv_numfmt_f6(double v) {
    if (!bv_numfmt_f6_ok(v)) return bv_numfmt_bad();
    const uint64_t bits = bv_numfmt_bits(v);
    uint64_t k; int32_t s;
    bv_numfmt_split(bits, &k, &s);
    bv_numfmt_val o = bv_numfmt_none();
    o.kind = BV_NUM_F6;
    o.neg = (uint8_t)(bits >> 63);
    if (s <= 0) {  // an integer below 2^63: s >= -10
        o.a = k << -s;
    } else if (s <= 74) {
        const uint64_t ip = s >= 53 ? 0ull : k >> s, f = s >= 53 ? k : k & ((1ull << s) - 1ull);
        const uint64_t fp = bv_numfmt_rhe_shift((bv_u128)f * 1000000ull, (uint32_t)s);
        o.a = ip + (fp == 1000000ull ? 1ull : 0ull);
        o.b = fp == 1000000ull ? 0u : (uint32_t)fp;
    }
    return o;
}

// 10^E <= k / 2^s, for -13 <= E <= 6 and 33 <= s <= 92
BV_NUMFMT_FN bool bv_numfmt_ge_pow10(uint64_t k, uint32_t s, int32_t E) {
    if (E >= 0) return (bv_u128)k >= ((bv_u128)bv_numfmt_pow10((uint32_t)E) << s);
    return (bv_u128)k * bv_numfmt_pow10((uint32_t)-E) >= ((bv_u128)1 << s);
}

BV_NUMFMT_FN bv_numfmt_val bv_numfmt_g6(double v) {
    if (!bv_numfmt_g6_ok(v)) return bv_numfmt_bad();
    const uint64_t bits = bv_numfmt_bits(v);
    bv_numfmt_val o = bv_numfmt_none();
    o.neg = (uint8_t)(bits >> 63);
    if ((bits & ~(1ull << 63)) == 0) {
        o.kind = BV_NUM_UINT;
        return o;
    }
    uint64_t k; int32_t s;
    bv_numfmt_split(bits, &k, &s);  // a normal: 2^t <= |v| < 2^(t+1) with t = 52 - s, -40 <= t <= 19
    // floor(t log10 2) or one more: t * 1233 / 4096 is that floor for |t| <= 40, and the comparison decides
    int32_t E = ((52 - s) * 1233) >> 12;
    if (bv_numfmt_ge_pow10(k, (uint32_t)s, E + 1)) ++E;
    uint64_t n = bv_numfmt_rhe_shift((bv_u128)k * bv_numfmt_pow10((uint32_t)(5 - E)), (uint32_t)s);
    if (n == 1000000ull) { n = 100000ull; ++E; }
    uint32_t nd = 6;
    while (nd > 1u && n % 10ull == 0) { n /= 10ull; --nd; }
    o.kind = BV_NUM_G6;
    o.b = (uint32_t)n; o.e = E; o.nd = (uint8_t)nd;
    return o;
}

BV_NUMFMT_FN uint32_t bv_numfmt_len(bv_numfmt_val x) {
    switch (x.kind) {
        case BV_NUM_UINT: return x.neg + bv_numfmt_digits(x.a);
        case BV_NUM_F6: return x.neg + bv_numfmt_digits(x.a) + 7u;
        case BV_NUM_G6: {
            const uint32_t nd = x.nd;
            if (x.e < -4) return x.neg + nd + (nd > 1u ? 1u : 0u) + 4u;
            if (x.e < 0) return x.neg + 1u + (uint32_t)-x.e + nd;
            return x.neg + (nd > (uint32_t)x.e + 1u ? nd + 1u : (uint32_t)x.e + 1u);
        }
        default: return 0;
    }
}

// the `n` low decimal digits of x to out[0 .. n), the most significant first
BV_NUMFMT_FN void bv_numfmt_put_digits(uint64_t x, uint32_t n, uint8_t *out) {
    for (uint32_t i = n; i-- > 0;) {
        out[i] = (uint8_t)('0' + (uint32_t)(x % 10ull));
        x /= 10ull;
    }
}

// writes bv_numfmt_len(x) bytes
BV_NUMFMT_FN void bv_numfmt_put(bv_numfmt_val x, uint8_t *out) {
    if (x.kind == BV_NUM_NONE || x.kind == BV_NUM_BAD) return;
    if (x.neg) *out++ = '-';
    if (x.kind == BV_NUM_UINT) {
        bv_numfmt_put_digits(x.a, bv_numfmt_digits(x.a), out);
    } else if (x.kind == BV_NUM_F6) {
        const uint32_t d = bv_numfmt_digits(x.a);
        bv_numfmt_put_digits(x.a, d, out);
        out[d] = '.';
        bv_numfmt_put_digits(x.b, 6u, out + d + 1u);
    } else {
        const uint32_t nd = x.nd;
        if (x.e < -4) {
            bv_numfmt_put_digits(x.b, nd, out + (nd > 1u ? 1u : 0u));  // d0 lands on out[1] ...
            if (nd > 1u) { out[0] = out[1]; out[1] = '.'; }            // ... and moves in front of the point
            uint8_t *t = out + nd + (nd > 1u ? 1u : 0u);
            t[0] = 'e'; t[1] = '-';
            bv_numfmt_put_digits((uint64_t)-x.e, 2u, t + 2);
        } else if (x.e < 0) {
            const uint32_t z = (uint32_t)-x.e - 1u;
            out[0] = '0'; out[1] = '.';
            for (uint32_t i = 0; i < z; ++i) out[2u + i] = '0';
            bv_numfmt_put_digits(x.b, nd, out + 2u + z);
        } else {
            const uint32_t ip = (uint32_t)x.e + 1u;  // digits in front of the point
            if (nd <= ip) {
                bv_numfmt_put_digits((uint64_t)x.b * bv_numfmt_pow10(ip - nd), ip, out);
            } else {  // the digits, then those behind the point move one place for it
                bv_numfmt_put_digits(x.b, nd, out);
                for (uint32_t i = nd; i > ip; --i) out[i] = out[i - 1u];
                out[ip] = '.';
            }
        }
    }
}

#endif  // BV_NUMFMT_CORE_H
