// bv_fused_solver.h -- the solver side of the fused short-row kernel: claiming candidates from the LDS queues, the 16-lane and the
// wave-solver jobs, the variant queue and its overflow list, and one unit of solver work (bv_f_solver_step).
// Included by bv_pass1_fused.hip alone, behind bv_fused_shared.h and bv_fused_lds.h; the kernel shell calls bv_f_solver_step;
// the variant-list flush and the wave-solver job on a site's exported bins are bv_short.h's.
#pragma once

// ------------------------------------------------------------------------------ the solver side
struct BvFusedSolver {
    BvSolveArgs sa;
    uint32_t *grp;   // this wave's four group scratches (LDS)
    uint32_t *vl;    // this wave's variant sites since the last flush (LDS)
    uint32_t n_vl;
    BvP1sWaveScratch *big;  // the wave solver's scratch, or NULL: this wave cannot take the hard candidates
    bool fuse2;      // variant sites also go to the workgroup's variant queue (their pass-2 rows are streamed by this kernel)
};
// claim `least` to `most` entries of a queue: returns the number claimed (0: too few there, or another wave was faster) and
// the first position
__device__ __forceinline__ uint32_t bv_f_claim(uint32_t *ctl, int tail_i, int head_i, uint32_t least, uint32_t most, uint32_t &first, int lane) {
    const uint32_t h = bv_f_lds_read_u(&ctl[head_i]), t = bv_f_lds_read_u(&ctl[tail_i]);
    if (t - h < least) return 0u;
    uint32_t n = t - h;
    if (n > most) n = most;
    uint32_t old = 0;
    if (lane == 0) old = atomicCAS(&ctl[head_i], h, h + n);
    old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
    first = h;
    return old == h ? n : 0u;
}
// the entry at `pos` (its producer reserved the position before writing it: wait for the site number), handed back empty
__device__ __forceinline__ uint32_t bv_f_take(uint32_t *q, uint32_t pos) {
    volatile __attribute__((address_space(3))) uint32_t *e = (volatile __attribute__((address_space(3))) uint32_t *)q + (pos & (BV_F_QCAP - 1u));
    uint32_t s = *e, spins = 0;
    while (s == BV_F_EMPTY && ++spins < BV_F_SPIN_MAX) { __builtin_amdgcn_s_sleep(4); s = *e; }
    *e = BV_F_EMPTY;
    return s;  // (BV_F_EMPTY after a time-out: the caller flags it)
}
// What the rank sums of pass 2 need of a variant site (bv_p2_site_facts, bv_pass2_sweep.h), the REF / ALT depths packed as the
// variant queue carries them: n1 | n2 << 16, both at most the row length (<= 49,152).
__device__ __forceinline__ void bv_f_p2_facts(int ref, const uint32_t depth[4], uint32_t aw0, uint32_t aw1, uint32_t &L, uint32_t &n12,
                                              uint32_t &lut) {
    uint32_t n1, n2;
    bv_p2_site_facts(ref, depth, aw0, aw1, L, lut, n1, n2);
    n12 = n1 | (n2 << 16);
}
// Variant sites into the workgroup's variant queue; called by the WHOLE wave, `want` marks the lanes that have one (their
// records are complete in memory).  The queue in LDS takes them while it is at most BV_F_QV_ROOM full: the positions are
// reserved in one atomic step per lane and counted at once, so whatever number of lanes of whatever number of waves pass that
// test together (at most 12 waves x 4), the queue cannot overflow and nobody ever waits for a slot of an entry that is not
// yet claimed.  Beyond that the sites go to the workgroup's OVERFLOW LIST in HBM (a.ovf: one 16-byte entry per site of the
// workgroup's range, so it cannot fill), appended by one wave at a time, published by the LDS word OV_TAIL behind an
// s_waitcnt that covers the entries' stores.
// Why not simply wait for room (as until round 5): the queue is emptied by the streaming waves, which themselves wait -- for
// room in the candidate queues that the solver waves empty, or, once past their pass-1 rows, inside this very function as
// solvers.  A workgroup with more variant sites in flight than the queue holds (few workgroups, many variants: 732 sites per
// workgroup in the campaign that found it) then stopped until the bounded waits gave up.  Now no solver ever waits on a
// streaming wave.
#define BV_F_QV_ROOM (BV_F_QVCAP - 48u)
__device__ __forceinline__ void bv_f_push_variants(const BvP1ShortArgs &a, BvFusedShared &sh, uint32_t B0, bool want, uint32_t site, uint32_t L,
                                                   uint32_t n12, uint32_t lut, int lane) {
    const unsigned long long m = __ballot(want);
    if (m == 0ull) return;
    if (bv_f_lds_read_u(&sh.ctl[BV_FC_QV_TAIL]) - bv_f_lds_read_u(&sh.ctl[BV_FC_QV_HEAD]) <= BV_F_QV_ROOM) {
        if (want) {
            const uint32_t pos = atomicAdd(&sh.ctl[BV_FC_QV_TAIL], 1u);
            volatile __attribute__((address_space(3))) uint32_t *e =
                (volatile __attribute__((address_space(3))) uint32_t *)&sh.qv[pos & (BV_F_QVCAP - 1u)][0];
            // (the entry that had this slot is claimed -- the occupancy test -- but its reader may be a few instructions from
            // handing the slot back)
            uint32_t spins = 0;
            while (e[0] != BV_F_EMPTY && spins < BV_F_SPIN_MAX) { __builtin_amdgcn_s_sleep(1); ++spins; }
            if (spins == BV_F_SPIN_MAX) atomicOr(&a.counters[BV_CTR_TIMEOUT], BV_TMO_PUSH_VARIANT);  // (nothing overwritten; loud)
            else {
                e[1] = L; e[2] = n12; e[3] = lut;
                e[0] = site;  // (LDS operations of one wave execute in order: the entry is whole when its site number appears)
            }
        }
        return;
    }
    // ---- the overflow list
    uint32_t spins = 0, got = 1u;
    do {
        if (lane == 0) got = atomicCAS(&sh.ctl[BV_FC_OV_LOCK], 0u, 1u);
        got = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
        if (got != 0u) __builtin_amdgcn_s_sleep(2);
    } while (got != 0u && ++spins < BV_F_SPIN_MAX);
    if (got != 0u) { if (lane == 0) atomicOr(&a.counters[BV_CTR_TIMEOUT], BV_TMO_PUSH_VARIANT); return; }
    const uint32_t base = bv_f_lds_read_u(&sh.ctl[BV_FC_OV_TAIL]);
    if (want) {
        uint32_t *e = a.ovf + 4u * (size_t)(B0 + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
        *reinterpret_cast<uint4 *>(e) = make_uint4(site, L, n12, lut);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the entries are in the L2 before their count says so
    if (lane == 0) {
        *(volatile __attribute__((address_space(3))) uint32_t *)&sh.ctl[BV_FC_OV_TAIL] = base + (uint32_t)__popcll(m);
        *(volatile __attribute__((address_space(3))) uint32_t *)&sh.ctl[BV_FC_OV_LOCK] = 0u;
    }
}

// four candidates, one per group of 16 lanes: positions first .. first + n - 1 of queue q
// A variant site enters the variant queue BETWEEN the two phases of its solve (bv_solver16.h): its rank-sum row needs the LRT's
// alleles only, and the jobs behind a workgroup's last pass-1 row are the end of the launch -- with the push behind phase 2 (until
// round 6) the last rows waited for the QUAL and the strand-bias tests of their sites too.  Phase 2 and the row's wave then write
// the same record at the same time: different fields, and the status word by atomic OR on both sides (phase 1 stores it whole).
__device__ __forceinline__ void bv_f_job16(const BvP1ShortArgs &a, BvFusedShared &sh, BvFusedSolver &v, uint32_t B0, uint32_t *q, uint32_t first,
                                           uint32_t n, int lane) {
    const int grp = lane >> 4, gl = lane & 15;
    uint32_t *scratch = v.grp + grp * BV_G16_GRP_WORDS;
    bool variant = false, live = false;
    uint32_t site = 0, pL = 0, pn12 = 0, plut = 0, nb = 0, badq = 0;
    const uint32_t *src = a.bins;
    BvG16Lrt pre;
    pre.status = 0; pre.aw0 = 0; pre.aw1 = 0; pre.chi2 = 0.; pre.ref = 4;
#ifdef BV_PHASE_DEBUG
    uint32_t jp_t_ = (uint32_t)__builtin_amdgcn_s_memtime(), jp_[6] = {0, 0, 0, 0, 0, 0};
#define BV_JP(i) do { const uint32_t n_ = (uint32_t)__builtin_amdgcn_s_memtime(); jp_[i] += n_ - jp_t_; jp_t_ = n_; } while (0)
#else
#define BV_JP(i)
#endif
    if ((uint32_t)grp < n) site = bv_f_take(q, first + (uint32_t)grp);
    if ((uint32_t)grp < n && site == BV_F_EMPTY) {
        if (gl == 0) atomicOr(&a.counters[BV_CTR_TIMEOUT], BV_TMO_TAKE);
    } else if ((uint32_t)grp < n) {
        live = true;
        src = a.bins + (size_t)site * BV_S_BIN_STRIDE;
        uint4 s0, s1, s2;
        bv_load3_l2(&a.summ[site], s0, s1, s2);
        BvG16Bins B;
        uint32_t depth[4] = {s0.x + s1.x, s0.y + s1.y, s0.z + s1.z, s0.w + s1.w};
        const uint32_t total = depth[0] + depth[1] + depth[2] + depth[3];
        nb = s2.x;
        badq = (s2.y & BV_SUM_BADQ) ? 1u : 0u;
        B.hit = sh.tab_hit; B.miss = sh.tab_miss; B.loghit = sh.tab_loghit; B.logmiss = sh.tab_logmiss;
        B.pm = reinterpret_cast<double *>(scratch) + gl;
#pragma unroll
        for (int s = 0; s < BV_G16_SLOTS; ++s) {
            const uint32_t i = (uint32_t)(s * 16 + gl);
            B.w[s] = i < nb ? src[i] : 0u;
        }
#ifdef BV_PHASE_DEBUG
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        BV_JP(0);  // the entry, the summary's and the bins' loads
        variant = bv_site_lrt_g16(v.sa, site, depth, total, badq, B, scratch, lane, &pre);
        if (variant && v.fuse2) bv_f_p2_facts(pre.ref, depth, pre.aw0, pre.aw1, pL, pn12, plut);
    }
    BV_JP(1);  // phase 1: the LRT and the record's first version
    const unsigned long long vm = __ballot(variant && gl == 0);
    if (variant && gl == 0) v.vl[v.n_vl + (uint32_t)__popcll(vm & ((1ull << lane) - 1ull))] = site;
    v.n_vl += (uint32_t)__popcll(vm);
    if (v.fuse2 && vm != 0ull) {
        // the records' first versions are complete (the rank sums' waves add to them)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bv_f_push_variants(a, sh, B0, variant && gl == 0, site, pL, pn12, plut, lane);
    }
    BV_JP(2);  // the record's stores complete, the variant sites queued
    if (live) {
        BvSiteSums S;
        // phase 2 needs the strand totals and, for the rank sum, the bins again (registers that would otherwise sit through the
        // EMs).  ONE trip: the bins' loads are issued first, and the summary load's own s_waitcnt vmcnt(0) covers them and the
        // stores of the record's first version, which phase 2 patches
        uint32_t w2[BV_G16_SLOTS];
#pragma unroll
        for (int s = 0; s < BV_G16_SLOTS; ++s) {
            const uint32_t i = (uint32_t)(s * 16 + gl);
            w2[s] = (variant && i < nb) ? src[i] : 0u;
        }
        uint4 s0, s1, s2;
        bv_load3_l2(&a.summ[site], s0, s1, s2);
        S.fwd[0] = s0.x; S.fwd[1] = s0.y; S.fwd[2] = s0.z; S.fwd[3] = s0.w;
        S.rev[0] = s1.x; S.rev[1] = s1.y; S.rev[2] = s1.z; S.rev[3] = s1.w;
        S.q0_mask = 0; S.nb = nb; S.badq = badq;
        BV_JP(3);  // phase 2's loads
        bv_site_tail_g16(v.sa, site, S, src, nb, scratch, lane, &pre, w2);
    }
    BV_JP(4);  // phase 2: rank sum, QUAL, strand-bias tests
    if (v.n_vl > 56u) bv_p1s_flush_vl(a, v.vl, v.n_vl, lane);
#ifdef BV_PHASE_DEBUG
    if (lane == 0) for (int i = 0; i < 5; ++i) atomicAdd(&a.counters[BV_CTR_WORDS + 4250 + i], jp_[i] >> 4);
#endif
#undef BV_JP
}
// one candidate that needs the wave solver (shallow site: ordered replay; phred-0 calls; more than 128 bins; min_af <= 0)
__device__ __forceinline__ void bv_f_job_hard(const BvP1ShortArgs &a, BvFusedShared &sh, BvFusedSolver &v, uint32_t B0, uint32_t site, int lane) {
    uint4 s0, s1, s2;
    bv_load3_l2(&a.summ[site], s0, s1, s2);
    BvSiteSums S;
    S.fwd[0] = s0.x; S.fwd[1] = s0.y; S.fwd[2] = s0.z; S.fwd[3] = s0.w;
    S.rev[0] = s1.x; S.rev[1] = s1.y; S.rev[2] = s1.z; S.rev[3] = s1.w;
    const uint32_t sm_nb = s2.x;
    S.q0_mask = s2.y & BV_SUM_Q0_MASK;
    S.badq = (s2.y & BV_SUM_BADQ) ? 1u : 0u;
    if (bv_p1s_hard_site(a, v.sa, site, S, sm_nb, v.big, sh.tab_hit, sh.tab_miss, lane)) {
        if (lane == 0) v.vl[v.n_vl] = site;
        ++v.n_vl;
        if (v.fuse2) {
            // the facts from the record as stored (read back through the L2: its stores are complete behind the wait)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            uint4 r0, r1, r2;
            bv_load3_l2(&a.out[site], r0, r1, r2);  // depth[4]; total, status, cvg_sb[0..1]; cvg_sb[2..3], cvg_fs
            const uint32_t *rw = reinterpret_cast<const uint32_t *>(&a.out[site].n_alt);
            const uint32_t aw0 = __builtin_nontemporal_load(rw), aw1 = __builtin_nontemporal_load(rw + 1);
            const uint32_t depth[4] = {r0.x, r0.y, r0.z, r0.w};
            int ref = v.sa.ref_base[site];
            if (ref > 4) ref = 4;
            uint32_t pL, pn12, plut;
            bv_f_p2_facts(ref, depth, aw0, aw1, pL, pn12, plut);
            bv_f_push_variants(a, sh, B0, lane == 0, site, pL, pn12, plut, lane);
        }
        if (v.n_vl > 56u) bv_p1s_flush_vl(a, v.vl, v.n_vl, lane);
    }
    bv_lrt_sync<0>();
}

// One unit of solver work, in this order: a job of candidates with three or four active bases (the longest jobs), a job of
// the others, (waves with the big scratch, once every streaming wave is past its last pass-1 row) a wave-solver candidate,
// a block of 64 non-candidate sites that every streaming wave has passed.  Returns 1: did something; 0: nothing to do right
// now; 2: nothing left to do, ever (no streaming wave will publish another pass-1 row, queues and blocks are empty -- jobs of
// other waves may still be running).
__device__ __forceinline__ int bv_f_solver_step(const BvP1ShortArgs &a, BvFusedShared &sh, BvFusedSolver &v, uint32_t B0, uint32_t B1,
                                                     int lane) {
    const uint32_t n_blocks = (B1 - B0 + 63u) >> 6;
    uint32_t first, n = 0;
    // (read before everything else: once every streaming wave is done, every block is ready and no candidate queue grows any more)
    const uint32_t n_done = bv_f_lds_read_u(&sh.ctl[BV_FC_NDONE]);
    // While rows are still streaming only FULL jobs are taken (four sites): a wave that runs off with the one candidate
    // that has just arrived spends a whole job on it, and the queue behind it grows -- the solver waves have ~60 % of the
    // streaming time's worth of work when every job is full.
    const uint32_t least = n_done == (uint32_t)BV_F_NS ? 1u : BV_F_MIN_JOB;
    // Is there anything to claim at all?  Only then is the wave counted in BUSY: a wave that merely polls must not hold the
    // count up -- the streaming waves wait for BUSY == 0 to know that no variant row is still to come (bv_f_no_row_ever), and
    // twelve waves polling through an unconditional count left it non-zero nearly all the time: a launch whose workgroups
    // all ran dry together (8 sites each) ended after SECONDS, whenever all counts happened to be down at once (round 5).
    const bool claimable = bv_f_lds_read_u(&sh.ctl[BV_FC_Q3_TAIL]) - bv_f_lds_read_u(&sh.ctl[BV_FC_Q3_HEAD]) >= least ||
                           bv_f_lds_read_u(&sh.ctl[BV_FC_Q2_TAIL]) - bv_f_lds_read_u(&sh.ctl[BV_FC_Q2_HEAD]) >= least ||
                           (v.big != nullptr && n_done == (uint32_t)BV_F_NS &&
                            bv_f_lds_read_u(&sh.ctl[BV_FC_QH_TAIL]) != bv_f_lds_read_u(&sh.ctl[BV_FC_QH_HEAD]));
    if (claimable) {
        // a job in flight is counted BEFORE its entries leave the queue (a wave that finds the queues empty and no job
        // counted knows that no variant site is still to come)
        if (lane == 0) atomicAdd(&sh.ctl[BV_FC_BUSY], 1u);
        uint32_t *q = sh.q3;
        n = bv_f_claim(sh.ctl, BV_FC_Q3_TAIL, BV_FC_Q3_HEAD, least, 4u, first, lane);
        if (n == 0u) { q = sh.q2; n = bv_f_claim(sh.ctl, BV_FC_Q2_TAIL, BV_FC_Q2_HEAD, least, 4u, first, lane); }
#ifdef BV_PHASE_DEBUG
        const uint32_t jt0_ = (uint32_t)__builtin_amdgcn_s_memtime();
#endif
        if (n != 0u) bv_f_job16(a, sh, v, B0, q, first, n, lane);   // (ONE call site: the solver is ~50 KB of code)
#ifdef BV_PHASE_DEBUG
        if (n != 0u && lane == 0) {
            const uint32_t dt_ = ((uint32_t)__builtin_amdgcn_s_memtime() - jt0_) >> 4, late_ = n_done == (uint32_t)BV_F_NS ? 4u : 0u;
            atomicAdd(&a.counters[BV_CTR_WORDS + 4212 + late_], dt_); atomicAdd(&a.counters[BV_CTR_WORDS + 4213 + late_], 1u);
            atomicAdd(&a.counters[BV_CTR_WORDS + 4214 + late_], n); if (q == sh.q3) atomicAdd(&a.counters[BV_CTR_WORDS + 4215 + late_], 1u);
        }
#endif
        if (n == 0u && v.big != nullptr && n_done == (uint32_t)BV_F_NS &&
            (n = bv_f_claim(sh.ctl, BV_FC_QH_TAIL, BV_FC_QH_HEAD, 1u, 1u, first, lane)) != 0u) {
            // (every streaming wave ran s_waitcnt vmcnt(0) behind its last list entry before it counted itself done)
            const uint32_t site = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_nontemporal_load(&a.cand_list[B0 + first]));
            bv_f_job_hard(a, sh, v, B0, site, lane);
        }
        if (lane == 0) atomicSub(&sh.ctl[BV_FC_BUSY], 1u);
#ifdef BV_TEAM_DEBUG  /* when the workgroup's last solver job ended */
        if (n != 0u && lane == 0) atomicMax(&a.counters[BV_CTR_WORDS + (blockIdx.x < 512u ? blockIdx.x : 511u) * 8u + 5u], (uint32_t)__builtin_amdgcn_s_memrealtime());
#endif
        if (n != 0u) return 1;
    }
    {
        const uint32_t bh = bv_f_lds_read_u(&sh.ctl[BV_FC_BLK_HEAD]);
        if (bh < n_blocks) {
            uint32_t ready = n_blocks;
            if (n_done < (uint32_t)BV_F_NS) {
                uint32_t m = 0xFFFFFFFFu;
#pragma unroll
                for (int w = 0; w < BV_F_NS; ++w) {
                    const uint32_t p = bv_f_lds_read_u(&sh.pub[w]);
                    m = p < m ? p : m;
                }
                ready = m >= B1 ? n_blocks : ((m - B0) >> 6);
            }
            if (bh < ready) {
                uint32_t old = 0;
                if (lane == 0) old = atomicCAS(&sh.ctl[BV_FC_BLK_HEAD], bh, bh + 1u);
                old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
                if (old == bh) {
                    const uint32_t site = B0 + bh * 64u + (uint32_t)lane;
                    if (site < B1) bv_p1s_simple_site<true>(a, v.sa.lnfact, site);
                }
                return 1;
            }
        }
    }
    if (n_done == (uint32_t)BV_F_NS) {
        // nothing was claimable a moment ago and no producer is left: done, unless a queue got its last entries in between
        const bool q_left = bv_f_lds_read_u(&sh.ctl[BV_FC_Q3_TAIL]) != bv_f_lds_read_u(&sh.ctl[BV_FC_Q3_HEAD]) ||
                            bv_f_lds_read_u(&sh.ctl[BV_FC_Q2_TAIL]) != bv_f_lds_read_u(&sh.ctl[BV_FC_Q2_HEAD]) ||
                            (v.big != nullptr && bv_f_lds_read_u(&sh.ctl[BV_FC_QH_TAIL]) != bv_f_lds_read_u(&sh.ctl[BV_FC_QH_HEAD])) ||
                            bv_f_lds_read_u(&sh.ctl[BV_FC_BLK_HEAD]) < n_blocks;
        if (!q_left && v.n_vl) bv_p1s_flush_vl(a, v.vl, v.n_vl, lane);
        return q_left ? 1 : 2;
    }
    return 0;
}
