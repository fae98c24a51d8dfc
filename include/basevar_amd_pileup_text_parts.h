/*
 * basevar_amd_pileup_text_parts.h -- batchfile rows over SAMPLE PARTS of one pileup.
 *
 * The reference cuts a cohort into batches of B samples and writes one batchfile per batch (_create_batchfiles,
 * src/basetype_caller.cpp:412-467).  bv_engine_pileup_text writes the rows of a whole tile; this call writes, from ONE wide
 * pileup, the rows of several column ranges of it -- each the text of a batchfile of its own (bv_pileup -B).  The bytes of a
 * part's row are defined at "ROWS OF A PART" in basevar_amd/csrc/bv_pileup_text_core.h; the kernels are the bv_pparts_ ones of
 * basevar_amd/csrc/bv_pileup_text.hip.
 *
 * basevar_amd_pileup_text.h includes this header: its calls continue that one's, and its fetch and deflate calls serve this text.
 */
#ifndef BASEVAR_AMD_PILEUP_TEXT_PARTS_H
#define BASEVAR_AMD_PILEUP_TEXT_PARTS_H

#include "basevar_amd_pileup_text.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bv_pileup_text_parts {
    const bv_pileup_text *rows; /* tile (or NULL: the last pileup), chrom, first_row, n_rows: as for bv_engine_pileup_text         */
    const uint32_t *part_first; /* host [n_parts + 1], strictly ascending, part_first[n_parts] <= n_samples;
                                   part p = samples [part_first[p], part_first[p + 1])                                            */
    uint32_t n_parts;           /* >= 1 */
    uint32_t reserved_;         /* must be 0 */
} bv_pileup_text_parts;

/* Format rows [first_row, first_row + n_rows) of every part into the engine's text buffer, PART-MAJOR: part 0's n_rows rows,
 * then part 1's, and so on.  The row of a part is bv_engine_pileup_text's row of a tile that holds only the part's columns: Depth
 * counts the claimed cells of those columns, the five lists run over them, and an indel cell takes the token of (pos, absolute
 * sample).  One part [0, n_samples) writes exactly bv_engine_pileup_text's bytes and offsets.  Parts need not cover all samples:
 * gaps before, between and behind them are allowed, and nothing of a gap's columns is looked at.
 * row_off[n_parts * n_rows + 1] (host): row k of part p is text[row_off[p * n_rows + k] .. row_off[p * n_rows + k + 1]),
 * row_off[0] = 0.  n_rows == 0: BV_OK, row_off[0] = 0, an empty text.
 * bv_engine_pileup_text_fetch and _deflate serve this text as they serve bv_engine_pileup_text's; a caller who wants no BGZF
 * member to span two parts passes a block_off that cuts at row_off[p * n_rows].  With tile == NULL the pileup stays usable by
 * bv_engine_pileup_rows / _submit afterwards.
 * Refusals, nothing launched and row_off unwritten: bv_engine_pileup_text's, and BV_ERR_INVALID_ARG for NULL in / rows /
 * part_first, n_parts == 0, an empty part, a boundary that is not ascending or lies beyond n_samples, reserved_ != 0.
 * BV_ERR_TOO_LARGE: n_rows x the tiles of all parts reaches 2^26 (a part's tiles are counted from its first column: a part of
 * up to bv_pileup_text_tile_samples() samples is one tile wherever it starts), or the token text of the rows reaches 2^31 bytes.
 * BV_ERR_DATA: an indel cell of the rows INSIDE A PART has no token -- found by the count pass, before any text is written; the
 * message names its pos and absolute sample.  Such a cell in a gap is not an error.  After an error the engine holds no text.
 * Blocks until row_off is written and the text is complete. */
int bv_engine_pileup_text_parts(bv_engine *e, const bv_pileup_text_parts *in, uint64_t *row_off, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BASEVAR_AMD_PILEUP_TEXT_PARTS_H */
