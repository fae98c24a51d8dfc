/*
 * basevar_amd_pileup_text.h -- batchfile rows written on the device from piled-up planes.
 *
 * The reference writes one row of text per position of a region, covered or not, with five lists of one token per sample
 * (__write_record_to_batchfile, src/basetype_caller.cpp:1027-1101); host/pileup.hpp's pileup_rows_text does that with one
 * string append per token.  Here the rows are expanded from the four planes and the indel tokens where bv_engine_pileup left
 * them in device memory (basevar_amd/csrc/bv_pileup_text.hip; the bytes are defined at the head of
 * basevar_amd/csrc/bv_pileup_text_core.h) and deflated from there (basevar_amd/csrc/bv_deflate.hip).
 *
 * Same conventions as basevar_amd_pileup.h, whose calls this header continues: plain C, BV_OK or a negative status,
 * bv_last_error() has the message, everything that can be checked on the host is checked before anything is launched.
 */
#ifndef BASEVAR_AMD_PILEUP_TEXT_H
#define BASEVAR_AMD_PILEUP_TEXT_H

#include "basevar_amd_pileup.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An explicit tile: the planes of bv_pileup_result for positions beg .. beg + rows - 1 and its indel tokens. */
typedef struct bv_pileup_tile {
    const uint8_t *cell, *qual, *mapq; /* [rows][pitch], host or device memory (mem_kind), 16-byte aligned                    */
    const uint16_t *rank;              /* [rows][pitch]; a cell is claimed <=> its rank is non-zero                           */
    const bv_pileup_token *tokens;     /* host [n_tokens], strictly ascending by (pos, sample)                                */
    const uint8_t *text;               /* host [text_bytes]: token k's text is text[text_off .. text_off + text_len)          */
    uint64_t pitch;                    /* >= n_samples, a multiple of 16; cells at or beyond n_samples are never read into
                                          the output                                                                          */
    uint64_t n_tokens, text_bytes;
    uint32_t beg, rows, n_samples;
    uint32_t mem_kind;                 /* BV_MEM_HOST | BV_MEM_DEVICE: where the four planes lie                              */
} bv_pileup_tile;

typedef struct bv_pileup_text {
    const bv_pileup_tile *tile; /* NULL: the engine's last completed bv_engine_pileup -- its planes, depths, tokens and text
                                   where they lie                                                                             */
    const char *chrom;          /* CHROM of every row: chrom_len bytes, 1 .. 255, no tab and no line break                    */
    uint32_t chrom_len;
    uint32_t first_row, n_rows; /* rows [first_row, first_row + n_rows) of the tile                                           */
    uint32_t reserved_;         /* must be 0 */
} bv_pileup_text;

/* Samples of one tile of the kernels' schedule (the tests place their edges around it). */
uint32_t bv_pileup_text_tile_samples(void);

/* Format rows [first_row, first_row + n_rows) of the tile back to back into a text buffer the engine owns (device memory, valid
 * until the next such call or the next bv_engine_pileup).  The row of position pos = beg + row is
 *   CHROM \t pos \t REF \t Depth \t M \t B \t Q \t R \t S \n
 * with REF the uploaded reference's byte at pos - 1 (letter case kept), Depth the row's cells of rank != 0 (for an explicit tile
 * counted by the kernel that counts them for bv_engine_pileup), and M B Q R S the samples' mapq, read base, quality, rank and
 * strand tokens joined by one space each: `0 N ! 0 .` for a cell of rank 0 whatever its other planes hold; else decimal mapq,
 * "ACGT"[c & 3] or N for BV_CELL_N or the cell's indel token's text, the byte (qual + 33) & 0xFF, decimal rank, and - for
 * c & BV_CELL_REV else +.  These are the bytes of host/pileup.hpp's pileup_rows_text.
 * row_off[n_rows + 1] (host) is written for the caller: row k is text[row_off[k] .. row_off[k + 1]), row_off[0] = 0.
 * n_rows == 0: BV_OK, row_off[0] = 0, and the engine then holds an empty text.  With tile == NULL the pileup stays usable by
 * bv_engine_pileup_rows / _submit afterwards.
 * BV_ERR_INVALID_ARG, nothing launched and row_off unwritten: NULL arguments, reserved_ != 0, a chrom_len outside 1 .. 255 or a
 * tab / line break in chrom, no reference set, a row beyond the reference, rows beyond the tile, tile == NULL without a completed
 * bv_engine_pileup; of an explicit tile a bad mem_kind, a pitch below n_samples or no multiple of 16, a NULL or misaligned plane,
 * tokens that are not strictly ascending by (pos, sample), a token whose text_off + text_len lies beyond text_bytes.
 * BV_ERR_TOO_LARGE: n_rows x tiles of a row reaches 2^26, or the token text of the rows reaches 2^31 bytes: format fewer rows a
 * call.  BV_ERR_DATA: an indel cell (BV_CELL_INS, BV_CELL_DEL; claimed) of the rows has no token -- found by the count pass,
 * before any text is written; the message names its pos and sample.  After an error the engine holds no text.
 * Blocks until row_off is written and the text is complete.
 * `stream`: a hipStream_t, or NULL for the engine's own; device planes must be complete on it. */
int bv_engine_pileup_text(bv_engine *e, const bv_pileup_text *in, uint64_t *row_off, void *stream);

/* Copy the formatted text, row_off[n_rows] bytes, to dst: bv_engine_vcf_fetch's contract (basevar_amd_vcf.h), with
 * bv_engine_pileup_text as the call that must come before. */
int bv_engine_pileup_text_fetch(bv_engine *e, void *dst, uint64_t dst_capacity, int dst_mem_kind, void *stream);

/* bv_engine_bgzf_deflate_level with the formatted text as its text: bv_engine_vcf_deflate's contract.  The members are the
 * bytes that call writes for the fetched text, at both levels. */
int bv_engine_pileup_text_deflate(bv_engine *e, const uint64_t *block_off, uint32_t n_blocks, int level, uint8_t *dst, uint64_t dst_capacity,
                                  uint64_t *member_off, void *stream);

#ifdef __cplusplus
}
#endif

/* rows over sample parts of one pileup, served by the fetch and deflate calls above: a header of its own */
#include "basevar_amd_pileup_text_parts.h"

#endif /* BASEVAR_AMD_PILEUP_TEXT_H */
