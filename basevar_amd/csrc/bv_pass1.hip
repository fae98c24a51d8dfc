// bv_pass1.hip -- pass 1 of the per-site basetype path: tally + solve, every site.
//
// Wave-specialised, persistent workgroups.  A workgroup is NTALLY tally waves + one solver wave
// (how a wave streams a row: bv_pass1_row.h; the ring they meet in: bv_pass1_ring.h; the tail of a launch: bv_pass1_team.h):
//
//   tally waves  stream one site (one slab row) after another, the row's 4 KiB blocks dealt
//                round-robin to the NTALLY waves: 16-byte coalesced, non-temporal loads of the
//                two byte planes along the sample axis (2 B/cell, each byte read exactly once),
//                software-pipelined (two sets of 4 KiB per plane, 16 KiB in flight per wave), covered
//                cells tallied with LDS atomics into a (strand, base, phred) histogram -- 8 KiB, one
//                of a small ring.  Sets that lie wholly inside the row take an unguarded fast path;
//                each 16-byte chunk is hand-scheduled (bv_tally_chunk).
//   solver wave  takes a finished histogram and runs the whole reference solver on it
//                (cites below), writes the site's 208-byte record, re-zeroes the histogram
//                and hands it back.
//
// The roles meet only through LDS sequence flags (published[] / filled[] / drained[]), never
// through s_barrier, so the HBM stream of site k+1 runs under the FP64 dependency chains of site k.
// (A first version that tallied and then solved with the same waves ran both phases in
// lock-step across the workgroups of a CU and reached 39 % of HBM peak; its tally alone
// ran at 75 %.  See DESIGN.md.)
//
// Reference functions realised here, all on the histogram:
//   BaseType ctor counts        src/basetype.cpp:45-71      -> depth[], total_depth
//   strand_bias (CVG flavour)   src/basetype.cpp:244-295    via caller.cpp:1236-1245
//   lrt(): EM / LRT / AF / QUAL src/basetype.cpp:130-199, src/algorithm.h:148-255
//   strand_bias (VCF flavour)   caller.cpp:1164
//   base-quality rank sum       src/basetype.cpp:201-242 via caller.cpp:1157
//   QD, CM_CAF                  caller.cpp:1122, 1160-1161
// HBM-bound by design; no inter-site reuse, so nothing to gain from an XCD-aware block
// remap (no two workgroups share a byte).  No MFMA: categorical tallies + small FP64 tables.
#include "bv_kernels.h"

#include "bv_solver.h"
#include "bv_tally.h"

#include "bv_pass1_ring.h"
#include "bv_pass1_row.h"
#include "bv_pass1_team.h"

// MODE 1: the team form -- the ticket rules and start-up below (first ticket = workgroup index, no ticket reserved while the
// solver is behind, phred tables fetched by the solver wave), and at the tail of the launch the tally waves help the solver
// wave (bv_pass1_team.h).  MODE 2: the same ticket rules and start-up without the helpers; the launches beyond
// BV_TEAM_MAX_SITES take it.  Nothing else is instantiated: the plain form both were measured against (MODE 0: every ticket an
// atomic, the tables copied in front of the start barrier) and workgroups of several solver waves (NSOLVE > 1, round 2: see
// bv_launch_pass1) are gone.  The parameter list stays as it was: the kernels' names are what the profiles and tools know them by.
template <int NTALLY, int NSOLVE, bool CHAIN = false, int MODE = 0>
__global__ __launch_bounds__(BV_WAVE *(NTALLY + NSOLVE), 4) void bv_pass1_kernel(BvPass1Args a) {
    static_assert(NSOLVE == 1 && (MODE == 1 || MODE == 2), "one solver wave; the team form or its ticket rules alone");
    constexpr bool TEAM = MODE == 1;
    constexpr int NT = BV_WAVE * (NTALLY + NSOLVE);
    constexpr int NBUF = NSOLVE + BV_RING_EXTRA;  // the tally may run BV_RING_EXTRA sites ahead of a slow (variant-site) solve
    __shared__ BvPass1Shared<NBUF> sh;
    BvTeam *const tm = bv_team_lds<TEAM>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    BV_TEAM_STAMP_INIT();
    BV_TEAM_STAMP(tid == 0, 0);  // entry
    // one-time set-up by the whole workgroup: zero the ring (the phred tables are the solver wave's to fetch)
    {
        uint4 *h4 = reinterpret_cast<uint4 *>(&sh.hist[0][0]);
        for (int i = tid; i < NBUF * BV_H2_WORDS / 4; i += NT) h4[i] = make_uint4(0, 0, 0, 0);
        if (tid < NBUF) {
            sh.published[tid] = 0u;
            sh.filled[tid] = 0u;
            sh.drained[tid] = 0u;
            sh.swz_of[tid] = 0u;
        }
        if (tid == 0) sh.dense_hint = 0u;
        if (TEAM && tid == 0) {
            tm->helpers = 0u; tm->last_site = BV_TEAM_NO_SITE; tm->gen = 0u; tm->done = 0u; tm->fv_go = 0u; tm->f_done = 0u;
            tm->lrt.bar = 0u; tm->lrt.err = &a.counters[BV_CTR_TIMEOUT];
        }
    }
    __syncthreads();
    BV_TEAM_STAMP(tid == 0, 1);  // start barrier passed

    BvSolveArgs sa;  // the solver wave's; in the team form the tally waves fill theirs when they turn helpers

    // Sites are handed out by a global ticket counter (a.counters[BV_CTR_TICKET], zeroed by the engine before
    // the launch): a workgroup that drew cheap hom-ref sites simply draws more, so the persistent
    // grid drains evenly whatever the batch size.  Which workgroup solves a site has no influence
    // on the site's record, so results stay bit-reproducible.
    if (wave < NTALLY) {
        // ------------------------------------------------ tally waves (wave 0 leads)
        // (s_setprio(1) / s_setprio(3) for this role were measured, twice: 0.5-2 % slower; priorities stay equal.)
        // Tickets are drawn `chunk` sites at a time: 1 for long rows (a reserved site is tens of microseconds of
        // work, so reserving more would lengthen the drain), 4 for short rows (one atomic per site on a single
        // address saturates at ~85 M/s).
        const uint32_t chunk = a.n_samples > 16384u ? 1u : 4u;
        // Team form: (1) a workgroup's FIRST ticket is its own index -- no atomic: the persistent grid starts all at once and
        // 1,024 draws on one address take 12 us (measured: first rows began 3-30 us after the launch); the counter hands
        // out the tickets from gridDim.x * chunk on.  (2) The next ticket is drawn ahead, under the current row's stream,
        // only while the ring has room for it: a workgroup whose solver is a full ring behind would otherwise sit on a
        // reserved site that any other workgroup could have started at once (measured on 8,192-site launches: the last
        // tally ended 85 us after the first workgroup had run out of work).
        const uint32_t t0 = gridDim.x * chunk;
        uint32_t next = blockIdx.x * chunk, cur = 0, end = 0;
        bool have = true;  // `next` holds a ticket
        for (uint32_t k = 0;; ++k) {
            const uint32_t buf = k % NBUF, gen = k / NBUF;
            uint32_t site;
            if (wave == 0) {
                if (cur == end) {
                    if (!have) {  // nothing was reserved: wait for room, then draw
                        bv_wait_flag(&sh.drained[buf], gen, &a.counters[BV_CTR_TIMEOUT]);
                        if (lane == 0) next = t0 + atomicAdd(&a.counters[BV_CTR_TICKET], chunk);
                    }
                    cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)next);
                    end = cur + chunk;
                    if (cur < a.n_sites) {
                        const uint32_t nk = k + chunk;  // the slot of the next draw's first row
                        // (not under the very first row either: the grid starts in step, the burst of draws would return
                        // -- in order -- ahead of every workgroup's first loads)
                        have = k != 0 && __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&sh.drained[nk % NBUF], __ATOMIC_RELAXED,
                                                                                              __HIP_MEMORY_SCOPE_WORKGROUP)) == (int)(nk / NBUF);
                        if (have && lane == 0) next = t0 + atomicAdd(&a.counters[BV_CTR_TICKET], chunk);  // in flight under these rows' stream
                    }
                }
                site = cur < a.n_sites ? cur : 0xFFFFFFFFu;
                ++cur;
#ifdef BV_TEAM_DEBUG
                const unsigned long long tw_ = __builtin_readcyclecounter();
#endif
                bv_wait_flag(&sh.drained[buf], gen, &a.counters[BV_CTR_TIMEOUT]);  // the solver has re-zeroed this slot
#ifdef BV_TEAM_DEBUG  /* cycles the tally waves of this workgroup stood still because the ring was full */
                if (TEAM && lane == 0) atomicAdd(&a.counters[BV_CTR_EASY], (uint32_t)((__builtin_readcyclecounter() - tw_) >> 6));
#endif
                // dense rows (the solver's last row had a quarter of its cells covered: coverage is a property of the cohort) take
                // the bank swizzle -- the lead wave decides for the slot, the other tally waves and the solver follow it
                const uint32_t swz_row = (a.flags & BV_FLAG_NO_DOM) ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&sh.dense_hint, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                if (lane == 0) { sh.site_of[buf] = site; sh.swz_of[buf] = swz_row; }
                // (BV_FLAG_FAULT_LOST_HANDOFF, tests: workgroup 0 never publishes its first slot -- the other tally waves must give
                // up after their bounded wait)
                if (!((a.flags & BV_FLAG_FAULT_LOST_HANDOFF) && blockIdx.x == 0u && k == 0u))
                    bv_set_flag(&sh.published[buf], gen + 1u);
            } else {
                bv_wait_flag(&sh.published[buf], gen + 1u, &a.counters[BV_CTR_TIMEOUT]);
                site = sh.site_of[buf];
            }
            if (site == 0xFFFFFFFFu) {
                bv_add_flag(&sh.filled[buf], lane);  // end of work: this slot is the solver's marker
                break;
            }
            const uint8_t *pb = a.bs, *pq = a.q;
            if (CHAIN && a.ch != nullptr) {  // a chained launch: the segment's (biased) planes
                const BvChainC ch = bv_chain_const(a.ch);
                const uint32_t sg = bv_chain_seg_uniform(ch, site);
                pb = ch->bs[sg]; pq = ch->q[sg];
            }
            BV_TEAM_STAMP(wave == 0 && lane == 0 && k == 0, 2);  // first row begins
            if (__builtin_amdgcn_readfirstlane((int)sh.swz_of[buf]) != 0)
                bv_tally_row_wave<NTALLY, true>(pb + (size_t)site * a.pitch, pq + (size_t)site * a.pitch, a.n_samples, sh.hist[buf], wave, lane);
            else
                bv_tally_row_wave<NTALLY, false>(pb + (size_t)site * a.pitch, pq + (size_t)site * a.pitch, a.n_samples, sh.hist[buf], wave, lane);
            if (TEAM && wave == 0) {
                // Was that this workgroup's last row?  (The next ticket was drawn a row ago and has long arrived.)  The solver
                // wave then waits the microsecond it takes the tally waves to report as helpers instead of starting alone.
                if (cur == end && !have && cur < a.n_sites) {
                    // nothing reserved (first row, or the ring was full when this row began): draw now if there is room
                    const uint32_t nk = k + 1u;
                    if (__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&sh.drained[nk % NBUF], __ATOMIC_RELAXED,
                                                                              __HIP_MEMORY_SCOPE_WORKGROUP)) == (int)(nk / NBUF)) {
                        if (lane == 0) next = t0 + atomicAdd(&a.counters[BV_CTR_TICKET], chunk);
                        have = true;
                    }
                }
                bool last = cur >= a.n_sites;
                if (!last && cur == end && have) last = (uint32_t)__builtin_amdgcn_readfirstlane((int)next) >= a.n_sites;
                if (last && lane == 0) tm->last_site = site;
            }
            bv_add_flag(&sh.filled[buf], lane);  // release: this wave's ds_add of the row are done
        }
        if (TEAM) {
            // ------------------------------------------------ the tail: help the solver wave with what is left in the ring
            BV_TEAM_STAMP(wave == 0 && lane == 0, 3);  // tally waves done
            sa = bv_solve_args(a);  // (here, not at the start: the table pointers are loads the first row must not wait for)
            bv_add_flag(&tm->helpers, lane);
            for (uint32_t job = 1;; ++job) {
                bv_wait_flag(&tm->gen, job, &a.counters[BV_CTR_TIMEOUT]);
                const uint32_t site = tm->site, buf = tm->buf;
                if (site == 0xFFFFFFFFu) break;
                if (CHAIN && a.ch != nullptr) {
                    const BvChainC ch = bv_chain_const(a.ch);
                    sa.ref_base = ch->ref_base[bv_chain_seg_uniform(ch, site)];
                }
                bv_team_help<NTALLY>(sa, site, wave + 1, job, sh.hist[buf], sh.sv[0].bin_code, sh.sv[0].bin_cnt, tm,
                                     sh.tab_hit, sh.tab_miss, lane);
            }
        }
    } else {
        // ------------------------------------------------ the solver wave
        // (s is 0, the only solver wave.  It stays a run-time index into sv[1]: with a constant one every LDS access of the solve
        // folds its address and all four instantiations change, 530 to 830 instructions each -- the kernel is held byte for byte.)
        const int s = wave - NTALLY;
        sa = bv_solve_args(a);
        // The phred tables are the solver's (and, later, its helpers'): fetched here, under the first row's stream.  Behind
        // the workgroup's start barrier they held every tally wave back by one loaded-memory latency (measured: 2 us on
        // the XCD that starts first, 5-12 us on the other seven -- 1,024 workgroups already have 50 MB of row loads queued).
        for (int i = lane; i < BV_QBINS; i += BV_WAVE) {
            sh.tab_hit[i] = a.tables->hit[i];
            sh.tab_miss[i] = a.tables->miss[i];
        }
        bv_lrt_sync<0>();
        BV_TEAM_STAMP(lane == 0, 4);  // phred tables in LDS
        uint32_t jobs = 0;  // team jobs handed out
        for (uint32_t k = (uint32_t)s;; k += NSOLVE) {
            const uint32_t buf = k % NBUF, gen = k / NBUF;
            bv_wait_flag(&sh.filled[buf], (gen + 1u) * NTALLY, &a.counters[BV_CTR_TIMEOUT]);
            const uint32_t site = sh.site_of[buf];
            if (site == 0xFFFFFFFFu) {
                BV_TEAM_STAMP(lane == 0, 5);  // solver wave done
                if (TEAM) {  // release the helpers
                    if (lane == 0) tm->site = 0xFFFFFFFFu;
                    bv_set_flag(&tm->gen, jobs + 1u);
                }
                break;
            }
            if (CHAIN && a.ch != nullptr) {
                const BvChainC ch = bv_chain_const(a.ch);
                const uint32_t sg = bv_chain_seg_uniform(ch, site);
                sa.ref_base = ch->ref_base[sg]; sa.out = ch->out[sg]; sa.bs = ch->bs[sg]; sa.q = ch->q[sg];
            }
            // a row tallied with the dense-row swizzle: back into its plain order before anybody reads it
            if (__builtin_amdgcn_readfirstlane((int)sh.swz_of[buf]) != 0) bv_hist_unswizzle<8, 8>(sh.hist[buf], lane);
            if (TEAM) {
                uint32_t *hist = sh.hist[buf], *bin_code = sh.sv[s].bin_code, *bin_cnt = sh.sv[s].bin_cnt;
                BvSolverScratch *sv = &sh.sv[s].sc;
                constexpr int REC_WORDS = (int)(sizeof(bv_site_result) / 4);
                if (lane < REC_WORDS) reinterpret_cast<uint32_t *>(&sv->res)[lane] = 0u;
                BvSiteSums S;
                S.q0_mask = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (hist[b << 8] + hist[(b | 4) << 8]) S.q0_mask |= 1u << b;
                bv_prologue_wave<false>(hist, bin_code, bin_cnt, lane, S.fwd, S.rev, &S.nb, &S.badq);
                bv_lrt_sync<0>();
                BvHqFromHist hq{hist};
                bool team = bv_team_takes(sa.flags, S);
                if (team) {
                    team = __hip_atomic_load(&tm->helpers, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == (uint32_t)NTALLY;
                    if (!team && tm->last_site == site) {  // they are on their way
                        bv_wait_flag(&tm->helpers, (uint32_t)NTALLY, &a.counters[BV_CTR_TIMEOUT]);
                        team = true;
                    }
                }
#ifdef BV_TEAM_DEBUG
                const unsigned long long t0_ = __builtin_readcyclecounter();
#endif
                if (team) {
                    ++jobs;
                    if (lane == 0) { tm->site = site; tm->buf = buf; tm->lrt.bar = 0u; }
                    bv_set_flag(&tm->gen, jobs);
                    BvTeamWork<NTALLY> work;
                    work.tm = tm; work.job = jobs; work.err = &a.counters[BV_CTR_TIMEOUT];
                    bv_site_solve<false, BvHqFromHist, false, BvTeamWork<NTALLY>>(sa, site, S, bin_code, bin_cnt, hq, sv, sh.tab_hit,
                                                                                 sh.tab_miss, lane, work);
                    bv_wait_flag(&tm->done, jobs * (uint32_t)NTALLY, &a.counters[BV_CTR_TIMEOUT]);  // nobody reads the slot any more
                } else {
                    bv_site_solve<false>(sa, site, S, bin_code, bin_cnt, hq, sv, sh.tab_hit, sh.tab_miss, lane);
                }
#ifdef BV_TEAM_DEBUG
                if (lane == 0) {  // (long rows leave the short-row list counters free)
                    const uint32_t dt = (uint32_t)((__builtin_readcyclecounter() - t0_) >> 6);
                    atomicAdd(&a.counters[team ? BV_CTR_CANDS : BV_CTR_EASY3], 1u);
                    atomicAdd(&a.counters[(team ? BV_CTR_CANDS : BV_CTR_EASY3) + 1], dt);
                }
#endif
            } else {
                bv_solve_site_wave<false>(sa, site, (BV_LDS uint32_t *)sh.hist[buf], (BV_LDS uint32_t *)sh.sv[s].bin_code,
                                          (BV_LDS uint32_t *)sh.sv[s].bin_cnt, (BV_LDS BvSolverScratch *)&sh.sv[s].sc,
                                          (BV_LDS const double *)sh.tab_hit, (BV_LDS const double *)sh.tab_miss, lane);
            }
            // what the next rows are likely to be: this one's depth (the record is still staged in the solver's scratch)
            if (lane == 0) sh.dense_hint = (sh.sv[s].sc.res.total_depth >= (a.n_samples >> 2)) ? 1u : 0u;
            // hand the slot back, zeroed
            uint4 *h4 = reinterpret_cast<uint4 *>(sh.hist[buf]);
#pragma unroll
            for (int i = 0; i < BV_H2_WORDS / 4 / BV_WAVE; ++i) h4[i * BV_WAVE + lane] = make_uint4(0, 0, 0, 0);
            bv_set_flag(&sh.drained[buf], gen + 1u);
        }
    }
}

// (Rows of at most 49,152 samples never come here: bv_pass1_short.hip / bv_pass1_fused.hip.  Round 1's form for them -- four
// independent waves per workgroup that each tally and solve their own site -- is in docs/history/.)
// NTALLY tally waves per workgroup; MODE 1: the team form, MODE 2: its ticket rules and start-up without the helpers
template <int NTALLY, int MODE>
static void bv_launch_pass1_cfg(const BvPass1Args &a, hipStream_t stream) {
    // Persistent grid: as many workgroups as stay resident (VGPR-limited to 16 waves per CU), never more than there are sites.
    constexpr int NSOLVE = 1;
    constexpr uint32_t by_vgpr = 16u / (NTALLY + NSOLVE);
    constexpr uint32_t by_lds = (uint32_t)((160u * 1024u) / sizeof(BvPass1Shared<NSOLVE + BV_RING_EXTRA>));
    uint32_t grid = (a.n_cu ? a.n_cu : 256u) * (by_vgpr < by_lds ? by_vgpr : by_lds);
    if (grid > a.n_sites) grid = a.n_sites;
    // (the chained form is an instantiation of its own: the headline kernel keeps its register allocation)
    const dim3 block(64 * (NTALLY + NSOLVE));
    if (a.ch != nullptr) hipLaunchKernelGGL((bv_pass1_kernel<NTALLY, NSOLVE, true, MODE>), dim3(grid), block, 0, stream, a);
    else hipLaunchKernelGGL((bv_pass1_kernel<NTALLY, NSOLVE, false, MODE>), dim3(grid), block, 0, stream, a);
}

void bv_launch_pass1(const BvPass1Args &a, hipStream_t stream) {
    // Three tally waves + one solver wave per workgroup, four workgroups per CU.  (Measured and dropped, round 2, as <NTALLY,
    // NSOLVE>: <3,2> 15-30 % slower, <2,1> 4 %, <7,1> and <5,1> 6 %.)  Several tally waves share a row: short per-site latency, short tail.  Up to
    // BV_TEAM_MAX_SITES per launch the team form is used: the last solves of a workgroup are spread over its idle tally waves
    // (8,192 sites: 0.351 -> 0.327 ms, 65,536: ~1 %).  Larger launches take the team form's ticket rules and start-up without
    // its helpers (MODE 2): 14 interleaved A/B runs at 131,072 sites x 100 k samples, pass 1 4.17 -> 4.12 ms (-1.1 %); with the
    // helpers too (MODE 1) it measured 0.5 % slower there.
    // (BV_FLAG_LONG_ROW_FORM(2), tests: the form without helpers whatever the launch size -- an independent realisation of the tail)
    // (what follows the 3 is MODE, not a number of solver waves: there is always one)
    if (a.n_sites <= (uint32_t)BV_TEAM_MAX_SITES && ((a.flags >> 8) & 0xFu) != 2u) bv_launch_pass1_cfg<3, 1>(a, stream);  // team form
    else bv_launch_pass1_cfg<3, 2>(a, stream);                                                                            // no helpers
}
