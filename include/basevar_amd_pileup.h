/*
 * basevar_amd_pileup.h -- BAM records piled up on the device: reads in, slab rows out.
 *
 * The reference spends its batchfile-creation phase on the pileup: per sample, the reads of a window in file order, the first
 * claim of a (sample, position) wins (__fetch_base_in_region, src/basetype_caller.cpp:876-1024).  host/pileup.hpp does that on
 * host threads into four host planes.  Here the samples' raw BAM records -- the bytes of the uncompressed BAM stream, in host or
 * in device memory -- are piled up by one wave per sample into planes the engine owns (basevar_amd/csrc/bv_pileup.hip; the
 * result is defined at the head of basevar_amd/csrc/bv_pileup_core.h), and the covered rows are gathered into a device slab
 * that bv_engine_submit takes.
 *
 * Same conventions as basevar_amd_vcf.h: plain C, BV_OK or a negative status, bv_last_error() has the message, everything that
 * can be checked on the host is checked before anything is launched.
 */
#ifndef BASEVAR_AMD_PILEUP_H
#define BASEVAR_AMD_PILEUP_H

#include "basevar_amd_bgzf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The records of n_samples samples for one window [beg, end] (1-based, inclusive) of reference `tid`.  Run r is
 * records[run_off[r] .. run_off[r + 1]): whole BAM records (block_size word + block) back to back, e.g. the records of one BAI
 * chunk of the sample's fetch of the window -/+ 200 bases.  The runs of a sample, in order, are its file order. */
typedef struct bv_pileup_reads {
    const uint8_t *records;     /* host or device memory (mem_kind); byte run_off[0] is records[run_off[0]]                    */
    const uint64_t *run_off;    /* host [n_runs + 1], ascending                                                                */
    const uint32_t *run_sample; /* host [n_runs], non-decreasing, each below n_samples; a sample may have no run               */
    uint64_t pitch;             /* cells of a row of the planes: >= n_samples, a multiple of 16                                */
    uint32_t n_runs, n_samples;
    int32_t tid;                /* the reference's number in the BAM headers                                                   */
    uint32_t region_beg, region_end; /* the whole region: the 500 kb steps are laid out from region_beg                        */
    uint32_t beg, end;          /* the window; it must lie inside one step and have at most bv_pileup_max_rows() rows          */
    int32_t mapq_thd;
    uint32_t mem_kind;          /* BV_MEM_HOST | BV_MEM_DEVICE: where `records` lies                                           */
    uint32_t reserved_;         /* must be 0 */
} bv_pileup_reads;

/* One indel token: the cell (pos, sample) is BV_CELL_INS or BV_CELL_DEL and its text -- '+' or '-', the anchor's reference base,
 * the inserted read letters or the deleted reference bases -- is text[text_off .. text_off + text_len). */
typedef struct bv_pileup_token {
    uint32_t pos, sample;
    uint64_t text_off;
    uint32_t text_len, reserved_;
} bv_pileup_token;

/* Where bv_engine_pileup_fetch copies the last pileup to; any pointer may be NULL (that part is not copied).  Capacities count
 * elements: cells of a plane, rows, tokens, bytes of text. */
typedef struct bv_pileup_result {
    uint8_t *cell, *qual, *mapq;   /* [rows][pitch]                                                                           */
    uint16_t *rank;                /* [rows][pitch]                                                                           */
    uint32_t *depth;               /* [rows]                                                                                  */
    bv_pileup_token *tokens;       /* sorted by (pos, sample)                                                                 */
    uint8_t *text;
    uint64_t cells_capacity, rows_capacity, tokens_capacity, text_capacity;
    uint64_t cells, rows, n_tokens, text_bytes; /* out: what the pileup holds (written also when the call refuses a capacity) */
    uint32_t mem_kind;             /* BV_MEM_HOST | BV_MEM_DEVICE: where the seven buffers lie                                 */
    uint32_t reserved_;            /* must be 0 */
} bv_pileup_result;

/* The most rows a window may have: one step of the reference's grid. */
uint32_t bv_pileup_max_rows(void);

/* The contig's bases as the host's load_fasta_sequence returns them, letter case kept: uploaded once, kept until the next such
 * call (len == 0 forgets them).  Blocks until they are uploaded. */
int bv_engine_pileup_set_reference(bv_engine *e, const char *seq, uint64_t len);

/* Pile the records up into planes [rows][pitch] that the engine owns, rows = end - beg + 1: cell (BV_CELL_*: base | strand; N, +
 * and - tokens carry the strand bit too), phred, mapq and read-position rank of the first read of the sample that claims the
 * position; a cell is claimed <=> its rank is non-zero.  Unclaimed cells, and all at or beyond n_samples, hold BV_CELL_N, 0, 0, 0.
 * Also depth[row] (claimed samples, a row reduction of rank != 0: no atomics, the result does not depend on scheduling), the
 * indel tokens, and *n_covered = rows of depth > 0.  n_runs == 0: BV_OK, every cell unclaimed.
 * BV_ERR_INVALID_ARG, nothing launched: NULL arguments, reserved_ != 0, no reference set, pitch, mem_kind, run_off out of order,
 * run_sample descending or beyond n_samples, a window that crosses the step grid laid out from region_beg or lies outside the
 * region.  BV_ERR_TOO_LARGE: more than bv_pileup_max_rows() rows.  BV_ERR_DATA: a damaged record -- a block_size below 32, a
 * record that overruns its run, n_cigar / l_seq beyond the block, a CIGAR that consumes more query bases than l_seq, an indel
 * whose anchor lies outside the reference (a deletion that runs past its end is clipped); the message names the first such
 * sample, its run and the byte offset.  BV_ERR_SITE: a match base inside the step that is none of A C G T N, with the host's
 * text.  After an error the engine holds no pileup.  Blocks until the result is complete.
 * `stream`: a hipStream_t, or NULL for the engine's own; device records must be complete on it. */
int bv_engine_pileup(bv_engine *e, const bv_pileup_reads *in, uint32_t *n_covered, void *stream);

/* Copy the last pileup out.  BV_ERR_INVALID_ARG, and no buffer written, without a completed bv_engine_pileup, for reserved_ != 0,
 * a bad mem_kind, or a capacity below what its non-NULL buffer has to take; cells / rows / n_tokens / text_bytes are written in
 * either case.  Blocks until the buffers are written. */
int bv_engine_pileup_fetch(bv_engine *e, bv_pileup_result *out, void *stream);

/* The covered rows (depth > 0) of the last pileup, in window order, as a slab of BV_MEM_DEVICE planes of the pileup's pitch,
 * ready for bv_engine_submit: ref_base from the uploaded reference (toupper, then BV_BASE_*), group_id NULL.  tagged != 0: the
 * ranks in the BV_SLAB_RPR_TAGGED layout; BV_ERR_INVALID_ARG if a rank of the pileup exceeds BV_RPR_TAG_MAX_RANK.  pos / depth
 * (host, *n_covered entries each, either may be NULL): the rows' 1-based positions and depths.  No covered row: n_sites == 0
 * and NULL planes.  The slab is valid until the engine's next bv_engine_pileup or _pileup_rows.  Blocks until it is complete. */
int bv_engine_pileup_rows(bv_engine *e, int tagged, bv_slab *slab, uint32_t *pos, uint32_t *depth);

/* bv_engine_submit of rows [first, first + n) of the slab that the last bv_engine_pileup_rows filled, for a host caller: the
 * records come back to host memory -- out [n], gout [n][n_groups] or NULL when n_groups == 0 --, and on request the rows' cell
 * and phred bytes, [n][n_samples] each (what host/vcf_emit.hpp's format_vcf_line reads).  group_id: host [n_samples] or NULL.
 * n at most the engine's max_sites.  BV_ERR_INVALID_ARG without a bv_engine_pileup_rows since the last pileup, for rows
 * beyond the slab, n == 0 or a NULL out; otherwise bv_engine_submit's statuses.  Blocks until the buffers are written. */
int bv_engine_pileup_submit(bv_engine *e, uint32_t first, uint32_t n, const uint8_t *group_id, uint32_t n_groups, bv_site_result *out,
                            bv_group_result *gout, uint8_t *cell, uint8_t *phred, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BASEVAR_AMD_PILEUP_H */
