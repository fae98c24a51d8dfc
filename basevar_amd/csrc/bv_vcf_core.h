// bv_vcf_core.h -- the per-sample GT:AB:SO:BP columns of a VCF record (bv_engine_vcf_format, include/basevar_amd_vcf.h), as
// inline functions that the device kernels (bv_vcf.hip) and a plain g++ harness (tests/cpp/vcf_lines_check.cpp) both compile,
// as bv_deflate_core.h and bv_inflate_core.h are.
//
// THE BYTES, defined without reference to lanes or tiles.  For line k over a row of n samples:
//   line_k   = head_k || for s in 0 .. n-1: '\t' || tok(cell[s], phred[s]) || '\n'
//   tok(c,q) = "./."                                                                       if c & BV_CELL_NOCALL
//            = G_k(c&3) || ':' || "ACGT"[c&3] || ':' || (c & BV_CELL_REV ? '-' : '+') || ':' || BP[q]       otherwise
//   G_k(b)   = "0/." if gt[k][b] == '0', else "./" || gt[k][b]        (gt[k][b]: '0' the REF base, '.' no allele of the record,
//                                                                       '1' .. '4' the record's ALT of that number)
//   BP[q]    = "%f" of 1.0 - exp(q * -0.23025850929940458), q = 0 .. 255: 8 characters each, "0.000000" .. "1.000000"
// so a sample costs BV_VCF_TOK_NOCALL = 4 or BV_VCF_TOK_CALL = 17 bytes with its tab, and
//   len_k = |head_k| + 4 n + 13 covered_k + 1.
// host/vcf_emit.hpp's format_vcf_line writes these bytes behind its head; the tests hold this file to it.
#ifndef BV_VCF_CORE_H
#define BV_VCF_CORE_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if defined(__HIPCC__)
#define BV_VCF_FN __host__ __device__ inline
#else
#define BV_VCF_FN inline
#endif

#define BV_VCF_TOK_NOCALL 4u
#define BV_VCF_TOK_CALL 17u
#define BV_VCF_BP_CHARS 8u
#define BV_VCF_CELL_NOCALL 0x08u  // BV_CELL_NOCALL (include/basevar_amd.h)
#define BV_VCF_CELL_REV 0x04u     // BV_CELL_REV

// is `c` one of the characters gt[k][b] may be
BV_VCF_FN bool bv_vcf_gt_char_ok(uint8_t c) { return c == '0' || c == '.' || (c >= '1' && c <= '4'); }

BV_VCF_FN bool bv_vcf_covered(uint8_t cell) { return (cell & BV_VCF_CELL_NOCALL) == 0; }
BV_VCF_FN uint32_t bv_vcf_token_bytes(uint8_t cell) { return bv_vcf_covered(cell) ? BV_VCF_TOK_CALL : BV_VCF_TOK_NOCALL; }
BV_VCF_FN uint64_t bv_vcf_line_bytes(uint64_t head_bytes, uint64_t n, uint64_t covered) {
    return head_bytes + BV_VCF_TOK_NOCALL * n + (BV_VCF_TOK_CALL - BV_VCF_TOK_NOCALL) * covered + 1u;
}

// '\t' || tok(cell, phred) to out (any address space a plain pointer reaches); returns its bytes.  gt: the line's four
// characters; bp: the 256 x 8 characters of BP.
BV_VCF_FN uint32_t bv_vcf_token(uint8_t cell, uint8_t phred, const uint8_t *gt, const uint8_t *bp, uint8_t *out) {
    out[0] = '\t';
    if (!bv_vcf_covered(cell)) {
        out[1] = '.'; out[2] = '/'; out[3] = '.';
        return BV_VCF_TOK_NOCALL;
    }
    const uint32_t b = cell & 3u;
    const uint8_t g = gt[b];
    out[1] = g == '0' ? '0' : '.';
    out[2] = '/';
    out[3] = g == '0' ? '.' : g;
    out[4] = ':';
    out[5] = (uint8_t)"ACGT"[b];
    out[6] = ':';
    out[7] = (cell & BV_VCF_CELL_REV) ? '-' : '+';
    out[8] = ':';
    for (uint32_t i = 0; i < BV_VCF_BP_CHARS; ++i) out[9u + i] = bp[(uint32_t)phred * BV_VCF_BP_CHARS + i];
    return BV_VCF_TOK_CALL;
}

// The serial line builder: line_k to out (room for bv_vcf_line_bytes(head_bytes, n, n)); returns its bytes.
BV_VCF_FN uint64_t bv_vcf_line(const char *head, uint64_t head_bytes, const uint8_t *cell, const uint8_t *phred, uint64_t n, const uint8_t *gt,
                               const uint8_t *bp, uint8_t *out) {
    uint64_t at = 0;
    for (; at < head_bytes; ++at) out[at] = (uint8_t)head[at];
    for (uint64_t s = 0; s < n; ++s) at += bv_vcf_token(cell[s], phred[s], gt, bp, out + at);
    out[at++] = '\n';
    return at;
}

// BP on the host: the expression of vcf_emit.hpp's bp_text.  False if an entry is not 8 characters (nothing can be laid out then).
inline bool bv_vcf_bp_table(uint8_t *bp /* [256 * BV_VCF_BP_CHARS] */) {
    for (int q = 0; q < 256; ++q) {
        char buf[352];
        const int len = snprintf(buf, sizeof buf, "%f", 1.0 - exp(q * -0.23025850929940458));
        if (len != (int)BV_VCF_BP_CHARS) return false;
        memcpy(bp + (size_t)q * BV_VCF_BP_CHARS, buf, BV_VCF_BP_CHARS);
    }
    return true;
}

#endif  // BV_VCF_CORE_H
