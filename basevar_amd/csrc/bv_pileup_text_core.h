// bv_pileup_text_core.h -- the text of batchfile rows (bv_engine_pileup_text, include/basevar_amd_pileup_text.h), as inline
// functions that the device kernels (bv_pileup_text.hip) and a plain g++ harness (tests/cpp/pileup_text_check.cpp) both compile,
// as bv_vcf_core.h is.
//
// THE BYTES, defined without reference to lanes or tiles.  The row of position pos (1-based) of a tile of n samples is
//   row    = CHROM '\t' dec(pos) '\t' REF '\t' dec(Depth) '\t' M '\t' B '\t' Q '\t' R '\t' S '\n'
//   CHROM  the caller's string;  REF = ref[pos - 1], the uploaded reference's byte, its letter case kept
//   Depth  the cells of the row with rank != 0
//   M B Q R S   n tokens each, of samples 0 .. n-1, joined by one ' '.  For a cell with rank == 0, whatever its other planes hold,
//          the tokens are  "0"  "N"  "!"  "0"  "."  ; for a claimed cell (c its cell byte) they are
//            M  dec(mapq)
//            B  "ACGT"[c & 3]                        if !(c & BV_CELL_NOCALL)
//               "N"                                   if c & BV_CELL_NOCALL and (c & 3) == 0   (BV_CELL_N)
//               the text of the cell's indel token   otherwise (BV_CELL_INS, BV_CELL_DEL): the token whose (pos, sample) equals
//                                                     the cell's; a cell without one is an error, not a byte
//            Q  the one byte (qual + 33) & 0xFF: a quality of 222 or more WRAPS out of the characters (222 gives the byte 0xFF,
//               223 gives 0x00, 255 gives 0x20), as `(char)(qual + 33)` does on the host
//            R  dec(rank)
//            S  '-' if c & BV_CELL_REV, else '+'
// This is pileup_rows_text() of host/pileup.hpp byte for byte, which tests/cpp/pileup_rows_check.cpp pins to the reference's
// writer.  Seen from one sample, every list takes the sample's token and ONE more byte -- the ' ' behind it, or behind the last
// sample the list's '\t' ('\n' for S) -- so
//   |row| = |head| + (sum of M tokens + n) + (sum of B tokens + n) + 2 n + (sum of R tokens + n) + 2 n,   head = CHROM .. Depth '\t'.
#ifndef BV_PILEUP_TEXT_CORE_H
#define BV_PILEUP_TEXT_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define BV_PTEXT_FN __host__ __device__ __forceinline__
#else
#define BV_PTEXT_FN inline
#endif

#define BV_PTEXT_CELL_NOCALL 0x08u  // BV_CELL_NOCALL (include/basevar_amd.h)
#define BV_PTEXT_CELL_REV 0x04u     // BV_CELL_REV
#define BV_PTEXT_LISTS 5u           // M B Q R S
#define BV_PTEXT_MAX_DEC 10u        // digits of a uint32_t

// One indel token as the kernels and the harness see it: the layout of bv_pileup_token (include/basevar_amd_pileup.h)
struct BvPtextToken {
    uint32_t pos, sample;
    uint64_t text_off;
    uint32_t text_len, reserved_;
};

BV_PTEXT_FN uint32_t bv_ptext_digits(uint32_t v) {
    uint32_t d = 1;
    while (v >= 10u) { v /= 10u; ++d; }
    return d;
}

// dec(v) to out; returns its digits
BV_PTEXT_FN uint32_t bv_ptext_dec(uint32_t v, uint8_t *out) {
    const uint32_t d = bv_ptext_digits(v);
    for (uint32_t i = d; i-- > 0;) { out[i] = (uint8_t)('0' + v % 10u); v /= 10u; }
    return d;
}

BV_PTEXT_FN bool bv_ptext_is_indel(uint8_t cell) { return (cell & BV_PTEXT_CELL_NOCALL) && (cell & 3u); }
// B of a claimed cell that is no indel
BV_PTEXT_FN uint8_t bv_ptext_base_char(uint8_t cell) { return (cell & BV_PTEXT_CELL_NOCALL) ? (uint8_t)'N' : (uint8_t)"ACGT"[cell & 3u]; }
BV_PTEXT_FN uint8_t bv_ptext_qual_char(uint8_t qual) { return (uint8_t)((qual + 33u) & 0xFFu); }
BV_PTEXT_FN uint8_t bv_ptext_strand_char(uint8_t cell) { return (cell & BV_PTEXT_CELL_REV) ? (uint8_t)'-' : (uint8_t)'+'; }
// the byte behind sample s's token in list `list` (0 .. 4) of a row of n samples
BV_PTEXT_FN uint8_t bv_ptext_sep(uint32_t list, uint32_t s, uint32_t n) { return s + 1u < n ? (uint8_t)' ' : list + 1u < BV_PTEXT_LISTS ? (uint8_t)'\t' : (uint8_t)'\n'; }

// The index of the token of cell (pos, sample) in tokens[0 .. n) (strictly ascending by (pos, sample)), or n if there is none
BV_PTEXT_FN uint64_t bv_ptext_find(const BvPtextToken *tokens, uint64_t n, uint32_t pos, uint32_t sample) {
    const uint64_t key = ((uint64_t)pos << 32) | sample;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        const uint64_t k = ((uint64_t)tokens[mid].pos << 32) | tokens[mid].sample;
        if (k < key) lo = mid + 1u; else hi = mid;
    }
    return lo < n && tokens[lo].pos == pos && tokens[lo].sample == sample ? lo : n;
}

BV_PTEXT_FN uint64_t bv_ptext_head_bytes(uint32_t chrom_len, uint32_t pos, uint32_t depth) {
    return (uint64_t)chrom_len + 1u + bv_ptext_digits(pos) + 1u + 1u + 1u + bv_ptext_digits(depth) + 1u;
}

// CHROM '\t' pos '\t' REF '\t' Depth '\t' to out (room for bv_ptext_head_bytes); returns its bytes
BV_PTEXT_FN uint64_t bv_ptext_head(const char *chrom, uint32_t chrom_len, uint32_t pos, uint8_t ref, uint32_t depth, uint8_t *out) {
    uint64_t at = 0;
    for (; at < chrom_len; ++at) out[at] = (uint8_t)chrom[at];
    out[at++] = '\t';
    at += bv_ptext_dec(pos, out + at);
    out[at++] = '\t';
    out[at++] = ref;
    out[at++] = '\t';
    at += bv_ptext_dec(depth, out + at);
    out[at++] = '\t';
    return at;
}

// The serial row builder.  cell / qual / mapq / rank: the row's n cells; tokens[0 .. n_tokens) + text: the tile's indel tokens.
// out == NULL only counts.  Returns the row's bytes, or 0 where an indel cell has no token: *bad_sample is that sample then.
BV_PTEXT_FN uint64_t bv_ptext_row(const char *chrom, uint32_t chrom_len, uint32_t pos, uint8_t ref, const uint8_t *cell, const uint8_t *qual,
                                  const uint8_t *mapq, const uint16_t *rank, uint32_t n, const BvPtextToken *tokens, uint64_t n_tokens,
                                  const uint8_t *text, uint8_t *out, uint32_t *bad_sample) {
    uint32_t depth = 0;
    for (uint32_t s = 0; s < n; ++s) depth += rank[s] != 0;
    uint8_t tmp[BV_PTEXT_MAX_DEC];
    uint64_t at = bv_ptext_head_bytes(chrom_len, pos, depth);
    if (out) bv_ptext_head(chrom, chrom_len, pos, ref, depth, out);
    for (uint32_t list = 0; list < BV_PTEXT_LISTS; ++list)
        for (uint32_t s = 0; s < n; ++s) {
            const bool claimed = rank[s] != 0;
            const uint8_t c = cell[s];
            uint32_t len = 1;
            const uint8_t *src = tmp;
            switch (list) {
            case 0: len = bv_ptext_dec(claimed ? mapq[s] : 0u, tmp); break;
            case 1:
                if (claimed && bv_ptext_is_indel(c)) {
                    const uint64_t t = bv_ptext_find(tokens, n_tokens, pos, s);
                    if (t == n_tokens) { *bad_sample = s; return 0; }
                    src = text + tokens[t].text_off; len = tokens[t].text_len;
                } else {
                    tmp[0] = claimed ? bv_ptext_base_char(c) : (uint8_t)'N';
                }
                break;
            case 2: tmp[0] = claimed ? bv_ptext_qual_char(qual[s]) : (uint8_t)'!'; break;
            case 3: len = bv_ptext_dec(claimed ? rank[s] : 0u, tmp); break;
            default: tmp[0] = claimed ? bv_ptext_strand_char(c) : (uint8_t)'.'; break;
            }
            if (out) {
                for (uint32_t i = 0; i < len; ++i) out[at + i] = src[i];
                out[at + len] = bv_ptext_sep(list, s, n);
            }
            at += (uint64_t)len + 1u;
        }
    return at;
}

// ROWS OF A PART (bv_engine_pileup_text_parts, include/basevar_amd_pileup_text_parts.h).  The row of position pos for the sample
// part [s0, s1) of a tile is the row above of a tile that holds only columns s0 .. s1-1: Depth is the claimed cells among those
// columns, the five lists run over those columns only (the part's last sample takes the list's '\t' or '\n'), and an indel cell
// takes the token of (pos, ABSOLUTE sample): tokens keep the tile's sample numbers.  Nothing else differs.  cell / qual / mapq /
// rank are the row's cells of the whole tile, indexed by absolute sample; columns outside [s0, s1) are not looked at.
// Returns the row's bytes, or 0 where an indel cell of the part has no token: *bad_sample is that absolute sample then.
BV_PTEXT_FN uint64_t bv_ptext_row_part(const char *chrom, uint32_t chrom_len, uint32_t pos, uint8_t ref, const uint8_t *cell, const uint8_t *qual,
                                       const uint8_t *mapq, const uint16_t *rank, uint32_t s0, uint32_t s1, const BvPtextToken *tokens,
                                       uint64_t n_tokens, const uint8_t *text, uint8_t *out, uint32_t *bad_sample) {
    const uint32_t n = s1 - s0;
    uint32_t depth = 0;
    for (uint32_t s = s0; s < s1; ++s) depth += rank[s] != 0;
    uint8_t tmp[BV_PTEXT_MAX_DEC];
    uint64_t at = bv_ptext_head_bytes(chrom_len, pos, depth);
    if (out) bv_ptext_head(chrom, chrom_len, pos, ref, depth, out);
    for (uint32_t list = 0; list < BV_PTEXT_LISTS; ++list)
        for (uint32_t s = s0; s < s1; ++s) {
            const bool claimed = rank[s] != 0;
            const uint8_t c = cell[s];
            uint32_t len = 1;
            const uint8_t *src = tmp;
            switch (list) {
            case 0: len = bv_ptext_dec(claimed ? mapq[s] : 0u, tmp); break;
            case 1:
                if (claimed && bv_ptext_is_indel(c)) {
                    const uint64_t t = bv_ptext_find(tokens, n_tokens, pos, s);
                    if (t == n_tokens) { *bad_sample = s; return 0; }
                    src = text + tokens[t].text_off; len = tokens[t].text_len;
                } else {
                    tmp[0] = claimed ? bv_ptext_base_char(c) : (uint8_t)'N';
                }
                break;
            case 2: tmp[0] = claimed ? bv_ptext_qual_char(qual[s]) : (uint8_t)'!'; break;
            case 3: len = bv_ptext_dec(claimed ? rank[s] : 0u, tmp); break;
            default: tmp[0] = claimed ? bv_ptext_strand_char(c) : (uint8_t)'.'; break;
            }
            if (out) {
                for (uint32_t i = 0; i < len; ++i) out[at + i] = src[i];
                out[at + len] = bv_ptext_sep(list, s - s0, n);
            }
            at += (uint64_t)len + 1u;
        }
    return at;
}

#endif  // BV_PILEUP_TEXT_CORE_H
