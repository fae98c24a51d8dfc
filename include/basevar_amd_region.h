/*
 * basevar_amd_region.h -- the rows of one region out of batchfiles that are still compressed.
 *
 * The reference's calling phase is region-driven: _variant_calling_unit runs tbx_itr_querys(tbx, region) on every batchfile
 * and takes one line per file per position (src/basetype_caller.cpp:559-601).  bv_engine_text_parse_bgzf (basevar_amd_bgzf.h)
 * takes "file f's p-th line" and never looks at POS.  This call takes the lines of a region instead: the caller seeks every
 * file to wherever its index says the region may begin (any member at or before the region's first line will do), and the
 * device, where the inflated text lies, drops the lines in front of the region, takes the region's, stops at its end and
 * checks that the files agree on the positions.
 *
 * Same conventions as basevar_amd.h: plain C, BV_OK or a negative status, bv_last_error() has the message.
 */
#ifndef BASEVAR_AMD_REGION_H
#define BASEVAR_AMD_REGION_H

#include "basevar_amd_bgzf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* CHROM == name[0 .. name_len) and beg <= POS <= end: 1-based, inclusive, 1 <= beg <= end */
typedef struct bv_text_region {
    const char *name;
    uint32_t name_len, beg, end;
    uint32_t reserved_; /* must be 0 */
} bv_text_region;

/* bv_engine_text_parse_bgzf on the region's lines.  All of that call's contract and refusals hold; what differs:
 *
 * Per file, the lines are the complete lines behind skip_bytes and then skip_lines, as that call counts them.  The head of a
 * line is CHROM (the bytes before its first tab) and POS (1 to 10 decimal digits between the first and second tab, value
 * <= 4,294,967,295); anything else is a malformed head.  A line is REACHED when CHROM == name and POS >= beg, and IN when it
 * is also <= end.  first[f] is the first reached line, n_in[f] the number of consecutive IN lines from there; the selection
 * ends at the first line that is not IN.  *n_positions = P = min(max_positions, cfg.max_sites, min over f of n_in[f]), and row
 * (p, f) is line first[f] + p.  row_state, the planes, bv_engine_text_submit, bv_engine_text_rows_fetch and
 * bv_engine_text_heads_fetch are bv_engine_text_parse_bgzf's on these rows.
 *
 * cursor[f] is the start of line first[f] + P: the lines in front of the region are consumed whether a position was taken or
 * not (a run without a reached line is consumed whole), so a caller that alternates reading and calling always makes
 * progress.  A file that moved has its skip_lines behind it; a file without a complete line behind its skip is left where
 * it was -- cursor[f] is the place of skip_bytes[f] and its skip_lines are still to be skipped.
 *
 * *region_done = 1 when every file has n_in[f] == P and either its terminating line lies in the run or at_end is 1: the
 * region has no further row.  0: come back from the cursors (with longer runs where P is 0).
 *
 * BV_ERR_DATA, with nothing parsed and nothing consumed, the engine usable as before, for
 *   - a malformed head at or before the line that ends a file's selection (anywhere in a run that has no such line); heads
 *     behind that line are not looked at.  The message names the file and the line's ordinal behind the skip;
 *   - a file whose lines of the region end (terminating line or at_end) while another file has IN lines beyond P, with
 *     P < min(max_positions, cfg.max_sites);
 *   - POS of row (p, f) != POS of row (p, 0).
 * This is what a tabix query returns on files sorted by position, the only kind an index can be built of.
 * BV_ERR_INVALID_ARG additionally for a NULL region or region_done, a NULL or empty name, beg == 0, beg > end and a non-zero
 * reserved_.  The definition in full stands at the head of basevar_amd/csrc/bv_text_region_core.h. */
int bv_engine_text_parse_bgzf_region(bv_engine *e, const bv_bgzf_rows *rows, const bv_text_region *region, const uint8_t *group_id,
                                     uint32_t n_groups, uint32_t *n_positions, uint8_t *row_state, bv_bgzf_cursor *cursor,
                                     uint32_t *region_done, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BASEVAR_AMD_REGION_H */
