// bv_pass1_team.h -- the tail of a long-row launch: the tally waves that have streamed their last row join the solver wave
// (BvTeam, the solver wave's work policy BvTeamWork, a helper's part bv_team_help) and the BV_TEAM_STAMP instrumentation.
// Included by bv_pass1.hip alone, behind bv_pass1_ring.h; used by the TEAM form of bv_pass1_kernel.
#pragma once

#include "bv_pass1_ring.h"

// ------------------------------------------------------------------------------ the tail of a launch: team solves
// When a workgroup has streamed its last row, its tally waves used to exit while the solver wave worked through what was
// left in the ring -- a whole solve (8 EM runs, two Fisher tests, QUAL, a rank sum: 40-70 us on one wave at 10^5
// samples) with the HBM pipes empty.  On a 131,072-site batch that is 1-2 % of the launch; on a single 8,192-site batch it
// was 23 % (0.363 ms against 0.280 ms for the tally alone).  In the TEAM form of the kernel the tally waves stay: waves
// 0 .. NTALLY-2 join the solver wave for the LRT (bv_lrt's team mode: the EM runs of a level are independent,
// basetype.cpp:151-169), the last tally wave runs the site's Fisher tests (the CVG one needs nothing from the LRT; the
// VCF one starts the moment the ALT set is known) while the solver wave does QUAL and the base-quality rank sum.  Every
// run is the same one-wave arithmetic whoever executes it, so records are byte-identical to the form without helpers
// (tests/test_gpu_parity.py::test_team_tail_...).  Hand-offs are LDS flags with bounded spins, like the rest of the kernel.
struct __attribute__((aligned(16))) BvTeam {
    BvLrtTeamShared lrt;  // LRT scratch + counting barrier of the team
    uint32_t helpers;     // tally waves that have finished streaming and wait for team jobs
    uint32_t last_site;   // the last site this workgroup streams (set by the lead tally wave once it knows)
    uint32_t gen;         // team jobs handed out so far (the job's number, from 1)
    uint32_t site, buf;   // the job; site == 0xFFFFFFFF: no more jobs
    uint32_t done;        // helper completions, NTALLY per job
    uint32_t fv_go, f_done;  // == job number once the VCF table is posted / the Fisher results are
    uint32_t vtab[4], ntab;
    uint32_t f_flags;
    double c_fs, c_sor, v_fs, v_sor;
};
#define BV_TEAM_NO_SITE 0xFFFFFFFEu
#define BV_TEAM_MAX_SITES 65536

template <bool TEAM>
__device__ __forceinline__ BvTeam *bv_team_lds() {
    __shared__ BvTeam tm;
    return &tm;
}
template <>
__device__ __forceinline__ BvTeam *bv_team_lds<false>() {
    return nullptr;
}

// bv_site_solve's work policy on the solver wave of a team job (role 0)
template <int NLRT>
struct BvTeamWork {
    BvTeam *tm;
    uint32_t job;
    uint32_t *err;
    mutable bool posted = false;
    __device__ __forceinline__ void post(const uint32_t v[4], int ntab, int lane) const {
        if (lane == 0) {
            tm->vtab[0] = v[0]; tm->vtab[1] = v[1]; tm->vtab[2] = v[2]; tm->vtab[3] = v[3];
            tm->ntab = (uint32_t)ntab;
        }
        bv_set_flag(&tm->fv_go, job);
        posted = true;
    }
    __device__ __forceinline__ void lrt(const BvBins &B, const uint32_t depth[4], uint32_t total, int nspec, int ref,
                                        double min_af, BvLrtShared *, int lane, BvLrtOut &L, uint32_t q0_mask) const {
        bv_lrt<NLRT>(B, depth, total, 0 | (1 << 3) | (2 << 6) | (3 << 9), nspec, ref, min_af, &tm->lrt.lrt, 0, lane, L, q0_mask);
    }
    __device__ __forceinline__ void tables_known(const uint32_t v[4], int ntab, int lane) const { post(v, ntab, lane); }
    __device__ __forceinline__ void strand_bias(const uint32_t[4], const uint32_t v[4], int ntab, int lane, const BvLnTab &,
                                                double &c_fs, double &c_sor, double &v_fs, double &v_sor,
                                                uint32_t &flags) const {
        if (!posted) post(v, ntab, lane);  // not a variant site: only the CVG table
        bv_wait_flag(&tm->f_done, job, err);
        c_fs = tm->c_fs; c_sor = tm->c_sor;
        if (ntab == 2) { v_fs = tm->v_fs; v_sor = tm->v_sor; }
        flags |= tm->f_flags;
    }
};

// Which sites a team takes: deep ones (the shallow-site replay, bv_em_ordered, is one wave's job) of a normal launch.
__device__ __forceinline__ bool bv_team_takes(uint32_t flags, const BvSiteSums &S) {
    const uint32_t total = S.fwd[0] + S.fwd[1] + S.fwd[2] + S.fwd[3] + S.rev[0] + S.rev[1] + S.rev[2] + S.rev[3];
    return total > (uint32_t)BV_ORD_MAX && !(flags & (BV_FLAG_TALLY_ONLY | BV_FLAG_SKIP_LRT | BV_FLAG_SKIP_FISHER));
}

// A tally wave's part in one team job.  role 1 .. NLRT-1: LRT; role NLRT: the Fisher tests.
template <int NLRT>
__device__ __forceinline__ void bv_team_help(const BvSolveArgs &a, uint32_t site, int role, uint32_t job, uint32_t *hist,
                                             uint32_t *bin_code, uint32_t *bin_cnt, BvTeam *tm, const double *tab_hit,
                                             const double *tab_miss, int lane) {
    BvSiteSums S;
    S.q0_mask = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (hist[b << 8] + hist[(b | 4) << 8]) S.q0_mask |= 1u << b;
    // (the bins are re-derived by every team wave: the same values land in the same words, no hand-off needed)
    bv_prologue_wave<false>(hist, bin_code, bin_cnt, lane, S.fwd, S.rev, &S.nb, &S.badq);
    bv_lrt_sync<0>();
    uint32_t depth[4], total = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        depth[b] = S.fwd[b] + S.rev[b];
        total += depth[b];
    }
    int ref = a.ref_base[site];
    if (ref > 4) ref = 4;
    if (role < NLRT) {
        BvBins B;
        B.code = bin_code; B.cnt = bin_cnt; B.skip_mask = 0u; B.hit = tab_hit; B.miss = tab_miss;
        B.loghit = a.loghit; B.logmiss = a.logmiss;
        B.nb = (int)S.nb;
        B.ord = nullptr; B.n_ord = 0;
        BvLrtOut L;
        bv_lrt<NLRT>(B, depth, total, 0 | (1 << 3) | (2 << 6) | (3 << 9), 4, ref, a.min_af, &tm->lrt.lrt, role, lane, L, S.q0_mask);
    } else {
        uint32_t t[4] = {0, 0, 0, 0};  // CVG table: alt = every non-ref base (caller.cpp:1236-1245)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b == ref) { t[0] += S.fwd[b]; t[1] += S.rev[b]; } else { t[2] += S.fwd[b]; t[3] += S.rev[b]; }
        }
        uint32_t fl = 0;
#pragma unroll 1
        for (int k = 0; k < 2; ++k) {
            if (k) {
                bv_wait_flag(&tm->fv_go, job, tm->lrt.err);
                if (tm->ntab != 2u) break;
                t[0] = tm->vtab[0]; t[1] = tm->vtab[1]; t[2] = tm->vtab[2]; t[3] = tm->vtab[3];
            }
            double fs, sor;
            bv_strand_bias_wave(t[0], t[1], t[2], t[3], lane, a.lnfact, &fs, &sor, &fl);
            if (lane == 0) {
                if (k) { tm->v_fs = fs; tm->v_sor = sor; } else { tm->c_fs = fs; tm->c_sor = sor; }
            }
        }
        if (lane == 0) tm->f_flags = fl;
        bv_set_flag(&tm->f_done, job);
    }
    bv_add_flag(&tm->done, lane);
}

// -DBV_TEAM_DEBUG (tools/experiments/r3_team_debug.sh): every workgroup of the team form stamps s_memrealtime (100 MHz) at six
// points of its life into the engine's spare counter blocks, the solver wave counts team jobs / solo solves and their cycles;
// bv_engine_wait prints the distribution.  This is how the start and the tail of a launch were taken apart.
#ifdef BV_TEAM_DEBUG
#define BV_TEAM_STAMP_INIT()                                                                                               \
    uint32_t *dbg_ = a.counters + BV_CTR_WORDS + (blockIdx.x < 640u ? blockIdx.x : 639u) * 8u; /* counter blocks 1.. are free */ \
    if (TEAM && tid == 0 && blockIdx.x == 0) a.counters[BV_CTR_WORDS + 5150] = 2u; /* whose stamps these are */                       \
    if (TEAM && tid == 0) dbg_[7] = __builtin_amdgcn_s_getreg((31 << 11) | 20) /* XCC_ID */
#define BV_TEAM_STAMP(COND, SLOT)                                                   \
    do {                                                                            \
        if (TEAM && (COND)) dbg_[SLOT] = (uint32_t)__builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define BV_TEAM_STAMP_INIT() do { } while (0)
#define BV_TEAM_STAMP(COND, SLOT) do { } while (0)
#endif
