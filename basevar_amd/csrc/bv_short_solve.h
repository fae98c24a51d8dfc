// bv_short_solve.h -- the solve kernel of the two-kernel short-row form: bv_p1s_solve16_kernel, its workgroup state and how its
// waves draw their jobs (BvP1sTickets, bv_p1s_job).
// Included by bv_pass1_short.hip alone, behind bv_short.h; launched by bv_launch_p1s_solve.
#pragma once

// ---- the ordinary candidates, four per wave: one site per group of 16 lanes (bv_solver16.h), in two phases -- the LRT,
// then everything that follows it (bv_site_lrt_g16 / bv_site_tail_g16).  Measured as two kernels too (one per phase, and a third
// for the non-candidates): 0.125 ms per 100 k sites against 0.105 ms for the one below -- two kernel boundaries and two tails more.
// Jobs (four sites of one list) are numbered with the sites of three or four active bases
// first (several times the EM runs: longest jobs first).  Jobs and workgroups are dealt to BV_TICKET_SLICES slices (job j and
// workgroup w belong to slice j, w mod BV_TICKET_SLICES); a wave's first job is its rank in the slice, every further one is
// drawn from the slice's ticket counter when the wave gets there -- no draw at the start of the kernel, where all waves
// would queue on one address (~88 M atomics/s: 35 us for 3072 waves), and eight addresses instead of one after that.
#define BV_P1S_SOLVE16_NW 4
struct __attribute__((aligned(16))) BvP1sSolve16Shared {
    double tab_hit[BV_QBINS], tab_miss[BV_QBINS];
    BvP1sWaveScratch ws[BV_P1S_SOLVE16_NW];
    uint32_t vl[BV_P1S_SOLVE16_NW][64];                    // the wave's variant sites since the last flush
};
#define BV_P1S_SOLVE16_OCC 3
struct BvP1sJob {
    const uint32_t *list;
    uint32_t idx;
    bool active;
};
// the k-th job of this wave's slice; its next k
struct BvP1sTickets {
    uint32_t slice, n_slices, slice_waves, k;
    uint32_t *ctr;
    __device__ __forceinline__ void init(uint32_t *counters_base, uint32_t wave) {
        n_slices = gridDim.x < BV_TICKET_SLICES ? gridDim.x : BV_TICKET_SLICES;  // (every slice needs a workgroup)
        slice = blockIdx.x % n_slices;
        const uint32_t slice_wgs = (gridDim.x - slice + n_slices - 1u) / n_slices;
        slice_waves = slice_wgs * BV_P1S_SOLVE16_NW;
        k = (blockIdx.x / n_slices) * BV_P1S_SOLVE16_NW + wave;
        ctr = counters_base + slice * BV_CTR_STRIDE;
    }
    __device__ __forceinline__ uint32_t job() const { return slice + n_slices * k; }
    __device__ __forceinline__ void next(int lane) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(ctr, 1u);
        k = slice_waves + (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    }
};
__device__ __forceinline__ BvP1sJob bv_p1s_job(const BvP1ShortArgs &a, uint32_t job, uint32_t n_easy, uint32_t n_easy3, int grp) {
    const uint32_t j3 = (n_easy3 + 3u) >> 2;
    BvP1sJob j;
    if (job < j3) { j.list = a.easy3_list; j.idx = job * 4u + (uint32_t)grp; j.active = j.idx < n_easy3; }
    else { j.list = a.easy_list; j.idx = (job - j3) * 4u + (uint32_t)grp; j.active = j.idx < n_easy; }
    return j;
}

// One kernel: a wave takes a job through both phases (the LRT's results stay in registers), and when the jobs are gone it
// takes blocks of 64 non-candidate sites, one per lane.  (lrt + tail + simple site: 60 KB of code, inside the instruction
// cache of 64 KB per pair of CUs; round 2's kernel was 207 KB -- two inlined copies of the Fisher test, the log-factorial
// series at ~60 call sites -- and 1.2 % of its instruction fetches missed.)
__global__ __launch_bounds__(BV_WAVE *BV_P1S_SOLVE16_NW, BV_P1S_SOLVE16_OCC) void bv_p1s_solve16_kernel(BvP1ShortArgs a) {
    __shared__ BvP1sSolve16Shared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n_easy = a.counters[BV_CTR_EASY], n_easy3 = a.counters[BV_CTR_EASY3];
    const uint32_t n_jobs = ((n_easy + 3u) >> 2) + ((n_easy3 + 3u) >> 2);
    for (int i = tid; i < BV_QBINS; i += BV_WAVE * BV_P1S_SOLVE16_NW) {
        sh.tab_hit[i] = a.tables->hit[i];
        sh.tab_miss[i] = a.tables->miss[i];
    }
    __syncthreads();
    BvSolveArgs sa = bv_solve_args(a);
    const int grp = lane >> 4, gl = lane & 15;
    uint32_t *scratch = sh.ws[wave].grp[grp], *vl = sh.vl[wave];
    uint32_t n_vl = 0;  // variant sites in vl[]
    // (a lambda around the one definition: its four call sites are the compiler's to inline or not, as they were; forced inline
    // at each of them the kernel spills two VGPRs)
    auto flush_vl = [&]() { bv_p1s_flush_vl(a, vl, n_vl, lane); };
    // ---- first the candidates only the wave solver takes (shallow sites replayed in sample order, phred-0 calls, more than 128
    // bins, min_af <= 0): none in most batches, all of them in a cohort of <= 64 samples.  Dealt round-robin over the grid's waves;
    // one wave, one site, the solver of bv_solver.h on the exported bins.  (A kernel of their own until round 3: mostly empty, it
    // still cost a launch, a kernel boundary and -- beside the other lane's kernels -- 50-110 us of workgroups queueing to leave.)
    {
        const uint32_t n_cand = a.counters[BV_CTR_CANDS];
        const uint32_t n_waves = gridDim.x * BV_P1S_SOLVE16_NW, gw = blockIdx.x * BV_P1S_SOLVE16_NW + (uint32_t)wave;
#pragma unroll 1
        for (uint32_t t = gw; t < n_cand; t += n_waves) {
            const uint32_t site = a.cand_list[t];
            const BvSiteSummary sm = a.summ[site];
            BvSiteSums S;
#pragma unroll
            for (int b = 0; b < 4; ++b) { S.fwd[b] = sm.fwd[b]; S.rev[b] = sm.rev[b]; }
            S.q0_mask = sm.flags & BV_SUM_Q0_MASK;
            S.badq = (sm.flags & BV_SUM_BADQ) ? 1u : 0u;
            if (bv_p1s_hard_site(a, sa, site, S, sm.nb, &sh.ws[wave], sh.tab_hit, sh.tab_miss, lane)) {
                if (lane == 0) vl[n_vl] = site;
                if (++n_vl > 60u) flush_vl();
            }
            bv_lrt_sync<0>();
        }
        if (n_vl) flush_vl();  // (the groups' scratch starts clean of the list logic either way; the flush keeps the phases apart)
    }
    BvP1sTickets tk;
    tk.init(a.counters + BV_CTR_TICKET_A, (uint32_t)wave);
    for (; tk.job() < n_jobs; tk.next(lane)) {
        const BvP1sJob jb = bv_p1s_job(a, tk.job(), n_easy, n_easy3, grp);
        // (s_setprio for the jobs of three or four active bases -- the kernel's critical path, one runs 50-83 us of the kernel's
        // 94 -- was measured: no change; their time is dependent-latency, not lost issue slots)
        bool variant = false;
        uint32_t site = 0;
        if (jb.active) {
            site = jb.list[jb.idx];
            const uint32_t *src = a.bins + (size_t)site * BV_S_BIN_STRIDE;
            uint32_t nb, badq;
            BvG16Lrt pre;
            {
                // phase 1 needs the depths only: the strand totals are read again for phase 2 (eight registers that would
                // otherwise sit through the EMs, in a kernel at its register limit)
                const BvSiteSummary sm = a.summ[site];
                uint32_t depth[4], total = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) { depth[b] = sm.fwd[b] + sm.rev[b]; total += depth[b]; }
                nb = sm.nb;
                badq = (sm.flags & BV_SUM_BADQ) ? 1u : 0u;
                BvG16Bins B;
                B.hit = sh.tab_hit; B.miss = sh.tab_miss; B.loghit = sa.loghit; B.logmiss = sa.logmiss;
                B.pm = reinterpret_cast<double *>(scratch) + gl;
#pragma unroll
                for (int s = 0; s < BV_G16_SLOTS; ++s) {
                    const uint32_t i = (uint32_t)(s * 16 + gl);
                    B.w[s] = i < nb ? src[i] : 0u;
                }
                variant = bv_site_lrt_g16(sa, site, depth, total, badq, B, scratch, lane, &pre);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the record's first version is out before phase 2 patches it
            BvSiteSums S;
            {
                const volatile BvSiteSummary *vs = &a.summ[site];
#pragma unroll
                for (int b = 0; b < 4; ++b) { S.fwd[b] = vs->fwd[b]; S.rev[b] = vs->rev[b]; }
            }
            S.q0_mask = 0; S.nb = nb; S.badq = badq;
            bv_site_tail_g16(sa, site, S, src, nb, scratch, lane, &pre);
        }
        // the wave's variant sites of this round, in group order
        const unsigned long long vm = __ballot(variant && gl == 0);
        if (variant && gl == 0) vl[n_vl + (uint32_t)__popcll(vm & ((1ull << lane) - 1ull))] = site;
        n_vl += (uint32_t)__popcll(vm);
        if (n_vl > 60u) flush_vl();
    }
    if (n_vl) flush_vl();
    // ---- the non-candidate sites, one lane per site, in blocks of 64 drawn like the jobs
    const uint32_t n_blocks = (a.n_sites + 63u) >> 6;
    BvP1sTickets tb;
    tb.init(a.counters + BV_CTR_TICKET_B, (uint32_t)wave);
    for (; tb.job() < n_blocks; tb.next(lane)) {
        const uint32_t site = tb.job() * 64u + (uint32_t)lane;
        if (site < a.n_sites) bv_p1s_simple_site(a, sa.lnfact, site);
    }
}
