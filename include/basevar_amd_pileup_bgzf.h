/*
 * basevar_amd_pileup_bgzf.h -- BAM files piled up from their BGZF members, still compressed.
 *
 * bv_engine_pileup (basevar_amd_pileup.h) takes the samples' raw BAM records, which a host thread has read and inflated with
 * zlib.  Here the host only reads: for each sample's fetch of the window it hands over the whole compressed members that a BAI
 * chunk (or the file) covers and the two cut points of the chunk -- where its first record begins inside the first member and
 * where it ends inside the last (basevar_amd/host/raw_members.hpp plans that).  The engine inflates the members with
 * bv_engine_bgzf_inflate's kernel into a buffer of its own and piles the records up where they lie.
 *
 * Same conventions as basevar_amd_pileup.h: plain C, BV_OK or a negative status, bv_last_error() has the message, everything
 * that can be checked on the host is checked before anything is launched.
 */
#ifndef BASEVAR_AMD_PILEUP_BGZF_H
#define BASEVAR_AMD_PILEUP_BGZF_H

#include "basevar_amd_pileup.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One run: consecutive whole members of one file and the records cut out of their text. */
typedef struct bv_pileup_bgzf_run {
    uint32_t sample;        /* non-decreasing over the runs, < n_samples; a sample may have no run */
    uint32_t first_member;  /* index into member_off */
    uint32_t n_members;     /* >= 1: consecutive members of one file, in file order */
    uint32_t begin;         /* inflated bytes into the FIRST member where the run's first record starts */
    uint32_t end;           /* inflated bytes of the LAST member that belong to the run */
    uint32_t reserved_;     /* must be 0 */
} bv_pileup_bgzf_run;

/* The members and runs of n_samples samples for one window; pitch, tid, region, window and mapq_thd as in bv_pileup_reads. */
typedef struct bv_pileup_bgzf {
    bv_bgzf_members members;          /* as bv_engine_bgzf_inflate takes them: host memory, whole members */
    const bv_pileup_bgzf_run *runs;   /* host [n_runs] */
    uint64_t pitch;
    uint32_t n_runs, n_samples;
    int32_t tid;
    uint32_t region_beg, region_end, beg, end;
    int32_t mapq_thd;
    uint32_t reserved_;
} bv_pileup_bgzf;

/* bv_engine_pileup on runs that are still compressed.  The engine inflates every member of `members` ONCE, back to back as
 * bv_engine_bgzf_inflate lays them out (dst_off[0] = 0, dst_off[k + 1] = dst_off[k] + member k's ISIZE field); run r is the bytes
 * from dst_off[first_member] + begin to dst_off[first_member + n_members - 1] + end: whole BAM records, which may lie across
 * member boundaries.  The runs of a sample, in order, are its file order.  Runs may name the same members (two BAI chunks that
 * meet inside one member).  The result is bv_engine_pileup's on those runs, byte for byte -- planes, depth, tokens, *n_covered --
 * and afterwards the engine holds a pileup exactly as after bv_engine_pileup: bv_engine_pileup_fetch, _rows and _submit and
 * bv_engine_pileup_text, _text_fetch and _text_deflate run unchanged behind it.  n_runs == 0: BV_OK, every cell unclaimed.
 *
 * MEMORY: the inflated text lies in one engine-owned device buffer of the sum of the members' ISIZE fields (+ 16 bytes, rounded
 * up to 256), grown on demand and kept between calls; it never shrinks before bv_engine_destroy.  The compressed bytes cross
 * through the pinned chunks of bv_engine_bgzf_inflate.
 *
 * BV_ERR_INVALID_ARG, nothing launched (every check needs the host bytes only; ISIZE is the member's last word): what
 * bv_engine_pileup refuses about its window, pitch, tid and reference; what bv_engine_bgzf_inflate refuses about its members; NULL
 * arguments, a reserved_ != 0; sample descending or beyond n_samples; n_members == 0 or members beyond members.n_members; begin
 * above the first member's ISIZE, end above the last member's; a one-member run with begin > end.  BV_ERR_TOO_LARGE as in
 * bv_engine_pileup.
 * BV_ERR_DATA, and the engine holds no pileup: a member whose status is not BV_BGZF_OK -- the message names the member's index,
 * its bv_bgzf_status and the first sample and run that use it; the statuses are read before the pile kernel is launched, which
 * never walks the bytes of a failed member (that is the call's one host wait before the pile) --, or a damaged record as in
 * bv_engine_pileup, with the sample, the run and the byte offset inside the run.  A cut point that lies inside a record (a
 * damaged index) ends there, as "a record overruns its run".  BV_ERR_SITE as in bv_engine_pileup.
 * Blocks until the result is complete.  `stream`: a hipStream_t, or NULL for the engine's own. */
int bv_engine_pileup_bgzf(bv_engine *e, const bv_pileup_bgzf *in, uint32_t *n_covered, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BASEVAR_AMD_PILEUP_BGZF_H */
