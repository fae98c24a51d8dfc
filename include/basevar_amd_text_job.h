/*
 * basevar_amd_text_job.h -- batchfile rows parsed a few files at a time: the parse job.
 *
 * bv_engine_text_parse (basevar_amd.h) takes one row of EVERY batchfile per position in one call, so its caller reads all files
 * side by side.  A cohort of thousands of batchfiles cannot be read that way: the readers outnumber the descriptors a process
 * may hold, and the batch shrinks to a few hundred positions.  A parse job runs over a window of P positions and takes the
 * files in groups: every add brings P rows of each of a run of adjacent files, and after the last add the engine holds what
 * bv_engine_text_parse leaves for the rows of all files joined position-major.  Everything behind a parse --
 * bv_engine_text_submit, the token list of basevar_amd_text_tokens.h, the record formatters -- follows unchanged.
 *
 * The parser's state is additive over files: a position's depth is a sum, its state an OR and its highest rank a maximum over
 * its rows, and file f writes only its own sample columns.  What bv_engine_text_parse asks of all files at once is that CHROM,
 * POS and REF of every row equal file 0's row of the position, and file 0 may come last here.  So the job keeps, per position,
 * the HEAD of the first row added for it: the row's bytes through its third tab, of which only the first 512 are looked at, as
 * bv_engine_text_parse looks at no more.  Every row, that first one included, is held to the head as bv_engine_text_parse holds
 * it to file 0's row, and ref[p] is taken where file 0's row passes.  This gives the whole parse's row_state: a position's state
 * is an OR over its rows, and all rows agree with file 0's row through their third tab exactly when all of them -- file 0's is
 * one -- agree with any one of them.  (Where they do not, the position is BV_TEXT_HOST either way; which of its rows were
 * refused is never seen.)
 *
 * Same conventions as basevar_amd.h: plain C, BV_OK or a negative status, bv_last_error() has the message.  With the token mode
 * off every call launches what bv_engine_text_parse launches for the same rows, plus the kernel that captures the heads.
 */
#ifndef BASEVAR_AMD_TEXT_JOB_H
#define BASEVAR_AMD_TEXT_JOB_H

#include "basevar_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Opens a job of n_positions x n_files rows; file f holds file_samples[f] samples, group_id / n_groups are
 * bv_engine_text_parse's.  Sizes and clears the planes and the heads.  An open job is abandoned; so is it by any
 * bv_engine_text_parse* call (a parse replaces the one before it).  The token mode (bv_engine_text_tokens_enable) is read here
 * and holds for the job.  BV_ERR_INVALID_ARG, the engine as it was: NULL file_samples, n_positions or n_files 0, n_positions
 * above cfg.max_sites, a file without samples, more samples than cfg.max_samples, group_id without 0 < n_groups <= BV_MAX_GROUPS
 * or the reverse. */
int bv_engine_text_job_begin(bv_engine *e, uint32_t n_positions, uint32_t n_files, const uint32_t *file_samples /*[n_files]*/,
                             const uint8_t *group_id, uint32_t n_groups, void *stream);

/* Adds files [first_file, first_file + rows->n_files): rows is a bv_text_rows as bv_engine_text_parse takes it, with the job's
 * n_positions; its row (p, k) is position p's line of file first_file + k, and rows->file_samples equals the job's entries for
 * those files.  Adds may come in any file order; every file is added exactly once.  Blocks until the text has been consumed:
 * the caller may free it.  row_flag (may be NULL; [n_positions][rows->n_files]) receives BV_TEXT_INDEL for every row of the add
 * that holds a '+SEQ' / '-SEQ' token and was parsed, 0 for every other.
 * BV_ERR_INVALID_ARG, the job as it was: no open job; n_positions or file_samples that differ from the job's; a file range
 * beyond n_files or one that touches a file already added; what bv_engine_text_parse refuses in a bv_text_rows (NULL pointers,
 * reserved_, offsets out of order or outside text_bytes, a row without its final '\n'); the token mode changed since begin.
 * Any other failure closes the job. */
int bv_engine_text_job_add(bv_engine *e, const bv_text_rows *rows, uint32_t first_file,
                           uint8_t *row_flag /* may be NULL: [n_positions][rows->n_files] */, void *stream);

/* After the last add: row_state [n_positions][n_files], the planes, the positions' highest ranks (which decide the tagged
 * layout), the group ids and, with the token mode on, the token list -- descriptors and text in (pos, file, sample) order,
 * whatever the order of the adds -- are what bv_engine_text_parse leaves, on the same engine, for the rows of all files joined
 * position-major.  bv_engine_text_submit follows as after any parse (n_positions_used, the host rows, one submit per parse).
 * BV_ERR_INVALID_ARG: no open job, NULL row_state; files still missing -- the job stays open and can be completed. */
int bv_engine_text_job_finish(bv_engine *e, uint8_t *row_state /*[n_positions][n_files]*/, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BASEVAR_AMD_TEXT_JOB_H */
