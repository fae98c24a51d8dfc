// bv_short.h -- pieces shared by the short-row pass-1 kernels (bv_pass1_short.hip: streaming kernel + solve kernel;
// bv_pass1_fused.hip: both in one persistent kernel): the histogram geometry, the one-lane finish of a non-candidate site
// (its per-lane Fisher test: bv_fisher.h), the streaming waves' histogram hand-back
// and list flush, the solver waves' variant-list flush, the wave solver's scratch and its job on a site's exported bins.
#pragma once

#include "bv_kernels.h"
#include "bv_solver.h"
#include "bv_solver16.h"
#include "bv_tally.h"

#define BV_S_HROWQ 128                       /* phred axis of the short-row histogram */
#define BV_S_HWORDS (BV_ROWS * BV_S_HROWQ)   /* 1024 words = 4 KiB */
#define BV_S_OVF 8                           /* + per-row counts of covered cells with phred >= 128 (invalid input) */
#define BV_S_SLOT_WORDS 512                  /* one slot of U = 1: 1 KiB of calls, then 1 KiB of phreds (U x that for U chunks per lane) */
#define BV_S_SIMPLE_MAX_TABLES 32            /* a non-candidate site's strand table has at most this many Fisher tables */

// ------------------------------------------------------------------------------ solve kernels
// A non-candidate site (hom-ref or uncovered), finished by ONE LANE: depths, flags, one small Fisher test.
// Three 16-byte loads served by the L2 (sc1: the CU's vector L1 is bypassed), waited for inside the statement.  For data that
// another wave of the SAME launch has stored (the fused kernel's hand-offs): summaries are 48 bytes, neighbours share a
// 128-byte line, and a line fetched for one site would otherwise be served stale from the L1 for the next.
__device__ __forceinline__ void bv_load3_l2(const void *p, uint4 &r0, uint4 &r1, uint4 &r2) {
    bv_u32x4 a, b, c;
    asm volatile(
        "global_load_dwordx4 %0, %3, off sc1\n\t"
        "global_load_dwordx4 %1, %3, off offset:16 sc1\n\t"
        "global_load_dwordx4 %2, %3, off offset:32 sc1\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(a), "=&v"(b), "=&v"(c)
        : "v"(p)
        : "memory");
    r0 = make_uint4(a.x, a.y, a.z, a.w); r1 = make_uint4(b.x, b.y, b.z, b.w); r2 = make_uint4(c.x, c.y, c.z, c.w);
}
// L2: the summaries were stored by other waves of this launch (bv_pass1_fused.hip)
template <bool L2 = false>
__device__ __forceinline__ void bv_p1s_simple_site(const BvP1ShortArgs &a, const BvLnTab &lnfact, uint32_t site) {
    const double qnan = __builtin_nan("");
    uint4 s0, s1, s2;
    if (L2) bv_load3_l2(&a.summ[site], s0, s1, s2);
    else {
        const uint4 *sp = reinterpret_cast<const uint4 *>(&a.summ[site]);
        s0 = sp[0]; s1 = sp[1]; s2 = sp[2];
    }
    if (s2.y & BV_SUM_CAND) return;
    const uint32_t fwd[4] = {s0.x, s0.y, s0.z, s0.w}, rev[4] = {s1.x, s1.y, s1.z, s1.w};
    bv_site_result r;
    {
        uint32_t *w = reinterpret_cast<uint32_t *>(&r);
#pragma unroll
        for (int i = 0; i < (int)(sizeof(r) / 4); ++i) w[i] = 0u;
    }
    uint32_t total = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) { r.depth[b] = fwd[b] + rev[b]; total += r.depth[b]; }
    r.total_depth = total;
    if (a.flags & BV_FLAG_TALLY_ONLY) {
        // diagnostic: depths only
    } else if (total == 0) {
        r.mq_ranksum = r.rpr_ranksum = r.bq_ranksum = qnan;  // caller.cpp:718 / basetype.cpp:132
    } else {
        int ref = a.ref_base[site];
        if (ref > 4) ref = 4;
        uint32_t flags = BV_SITE_COVERED | ((s2.y & BV_SUM_BADQ) ? BV_SITE_BAD_QUAL : 0u);
        uint32_t c_rf = 0, c_rr = 0, c_af = 0, c_ar = 0;  // caller.cpp:1236-1245
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b == ref) { c_rf += fwd[b]; c_rr += rev[b]; } else { c_af += fwd[b]; c_ar += rev[b]; }
        }
        if (!(a.flags & BV_FLAG_SKIP_FISHER)) {
            bv_strand_bias_tail(bv_fisher_two_sided_lane((int)c_rf, (int)c_rr, (int)c_af, (int)c_ar, lnfact), c_rf, c_rr, c_af, c_ar,
                                &r.cvg_fs, &r.cvg_sor, &flags);
            r.cvg_sb[0] = c_rf; r.cvg_sb[1] = c_rr; r.cvg_sb[2] = c_af; r.cvg_sb[3] = c_ar;
        }
        r.status = flags;
        // lrt() with one active base, the reference base: no ALT, chi2 0, one EM run of one iteration (bv_lrt)
        const bool lrt_ran = !(a.flags & BV_FLAG_SKIP_LRT);
        r.em_iters = lrt_ran ? 1 : 0;
        r.n_em = lrt_ran ? 1 : 0;
        r.mq_ranksum = r.rpr_ranksum = r.bq_ranksum = qnan;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(&a.out[site]);
    const uint4 *src = reinterpret_cast<const uint4 *>(&r);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(r) / 16); ++i) dst[i] = src[i];
}

// ------------------------------------------------------------------------------ streaming waves: steps of a row's epilogue
// (Its other steps -- the row's totals, the candidate test, the bins' compaction, the 12-lane summary store -- are written out in
// bv_p1s_stream_kernel and in bv_f_stream_until_idle, the same text except where the reference base comes from and where a
// candidate's bins go: as shared functions they moved the fused kernel's streaming loops by 2 % of their instructions, and both
// kernels' register allocation is tuned to the instruction.  Tried again with the pass-1 split (profiles/pass1_split_codehash.txt):
// the totals as a function cost bv_p1s_stream_kernel a VGPR, the other three steps 1.5-2.3 % of its run time.  A fix to one copy
// goes into the other.)
// hand a wave's histogram back zeroed: its 8 x 128 words (OVF: and the overflow rows behind them)
template <bool OVF>
__device__ __forceinline__ void bv_p1s_zero_hist(uint32_t *hist, int lane) {
    uint4 *h4 = reinterpret_cast<uint4 *>(hist);
#pragma unroll
    for (int i = 0; i < BV_S_HWORDS / 4 / BV_WAVE; ++i) h4[i * BV_WAVE + lane] = make_uint4(0, 0, 0, 0);
    if (OVF && lane < 2) h4[BV_S_HWORDS / 4 + lane] = make_uint4(0, 0, 0, 0);
}
// flush a wave's list of n <= 64 sites (lane k holds the k-th): one atomic reserves their places in `list`
__device__ __forceinline__ void bv_p1s_flush_list(uint32_t *counter, uint32_t *list, uint32_t mine, uint32_t n, int lane) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(counter, n);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if ((uint32_t)lane < n) list[base + (uint32_t)lane] = mine;
}

// ------------------------------------------------------------------------------ solver waves
// flush a wave's variant sites vl[0 .. n_vl) into the launch's variant list: one atomic reserves their places
__device__ __forceinline__ void bv_p1s_flush_vl(const BvP1ShortArgs &a, const uint32_t *vl, uint32_t &n_vl, int lane) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&a.counters[BV_CTR_VARIANTS], n_vl);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    bv_lrt_sync<0>();
    if ((uint32_t)lane < n_vl) a.var_list[base + (uint32_t)lane] = vl[lane];
    bv_lrt_sync<0>();
    n_vl = 0;
}

// Candidates that need the wave solver (shallow sites, phred-0 calls, > 128 bins, min_af <= 0): one wave per site.
#define BV_P1S_RAW_WORDS (2 * BV_SLOTS * BV_WAVE + 4 * 128)  /* the wave solver's per-wave bins: codes [384], counts [384], merged counts [4][128] */
// per wave: the four groups' scratch of the 16-lane solver -- or, while the wave works off the (rare) candidates that need the
// wave solver, that solver's bins and scratch in the same bytes
union __attribute__((aligned(16))) BvP1sWaveScratch {
    uint32_t grp[4][BV_G16_GRP_WORDS];  // per group: bv_site_lrt_g16 / bv_site_tail_g16
    struct {
        uint32_t raw[BV_P1S_RAW_WORDS];  // bin codes [384], bin counts [384], merged (base, phred) counts [4][128]
        BvSolverScratch sc;
    } w;
};
// One such candidate on one wave, from what its summary says (S: the strand totals, q0_mask, badq; sm_nb exported bins): the
// solver of bv_solver.h on the bins.  Returns whether the site is a variant site (the caller lists it).
__device__ __forceinline__ bool bv_p1s_hard_site(const BvP1ShortArgs &a, BvSolveArgs &sa, uint32_t site, BvSiteSums &S, uint32_t sm_nb,
                                                 BvP1sWaveScratch *ws, const double *tab_hit, const double *tab_miss, int lane) {
    uint32_t *bin_code = ws->w.raw, *bin_cnt = bin_code + BV_SLOTS * BV_WAVE, *hq = bin_code + 2 * BV_SLOTS * BV_WAVE;
    BvSolverScratch *sv = &ws->w.sc;
    constexpr int REC_WORDS = (int)(sizeof(bv_site_result) / 4);
    if (lane < REC_WORDS) reinterpret_cast<uint32_t *>(&sv->res)[lane] = 0u;
    {
        uint4 *z = reinterpret_cast<uint4 *>(hq);
#pragma unroll
        for (int i = 0; i < 4 * 128 / 4 / BV_WAVE; ++i) z[i * BV_WAVE + lane] = make_uint4(0, 0, 0, 0);
    }
    bv_lrt_sync<0>();
    // exported bins -> merged counts for the rank sum (all of them) and the EM's bins (phred <= 93), order kept
    const uint32_t *src = a.bins + (size_t)site * BV_S_BIN_STRIDE;
    uint32_t nb = 0;
    for (uint32_t i0 = 0; i0 < sm_nb; i0 += BV_WAVE) {
        const uint32_t i = i0 + (uint32_t)lane;
        const bool have = i < sm_nb;
        const uint32_t w = have ? src[i] : 0u;
        const uint32_t code = w >> 16, cnt = w & 0xFFFFu;
        if (have) hq[code] = cnt;
        const bool valid = have && (code & 127u) < BV_NQ_VALID;
        const unsigned long long m = __ballot(valid);
        const uint32_t pos = nb + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (valid) { bin_code[pos] = code; bin_cnt[pos] = cnt; }
        nb += (uint32_t)__popcll(m);
    }
    S.nb = nb;
    bv_lrt_sync<0>();
    BvHqMerged H{hq};
    if (a.ch != nullptr) {  // chained launch: the ordered gather of a shallow site reads the segment's (biased) planes
        const BvChainC ch = bv_chain_const(a.ch);
        const uint32_t sg = bv_chain_seg_uniform(ch, site);
        sa.bs = ch->bs[sg]; sa.q = ch->q[sg];
    }
    return bv_site_solve<false, BvHqMerged, true>(sa, site, S, bin_code, bin_cnt, H, sv, tab_hit, tab_miss, lane);
}
