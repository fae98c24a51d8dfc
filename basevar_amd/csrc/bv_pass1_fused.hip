// bv_pass1_fused.hip -- short rows (4,097 .. 49,152 samples per site): pass 1 and the variant sites' pass-2 rows as ONE
// persistent kernel.
//
// bv_pass1_short.hip + bv_pass2.hip run these rows as three launches -- a streaming kernel, a solve kernel, the rank-sum
// kernel of pass 2: while the first and third run the chip's vector units are ~40 % busy, while the second runs HBM is idle,
// and its 0.10 ms per 100 k sites (16 % of the step at 10 k samples) is fully exposed.  Here all three are roles of one
// workgroup of 12 waves (one per CU, three per SIMD):
//
//   waves 0-7  (stream)  draw sites from the workgroup's cursor and stream their rows through private LDS rings filled
//                        by LDS-DMA, exactly one site per draw, three 4 KiB slots in flight per wave across row
//                        boundaries.  The per-slot control is straight-line scalar code (two asm blocks: a full slot, a
//                        row's last slot with two precomputed exec masks) -- the streaming kernel of bv_pass1_short.hip
//                        spends ~110 scalar instructions and ~15 branches per slot on the same job.  Per row: the
//                        strand x base totals, the candidate test, ONE 48-byte summary store; a candidate's bins leave
//                        through a 512-byte LDS stage as two 64-lane stores.  A row's stores are counted: the three slot
//                        waits that follow it allow exactly that many more operations outstanding (s_waitcnt vmcnt(8 + S)),
//                        so a candidate row no longer drains the ring.
//   waves 8-11 (solve)   take the candidates from two queues in LDS (three or four active bases first), four sites per
//                        wave on 16-lane groups (bv_solver16.h), and finish the non-candidate sites one lane per site in
//                        blocks of 64 as soon as every streaming wave has passed them.  A variant site goes into a third
//                        queue with what its rank sums need (class table, REF / ALT depths) -- between the two phases of
//                        its solve: the LRT decides the alleles, QUAL and the strand-bias tests then run beside the site's row.
//   pass-2 rows          (FUSE2: rank planes given) a wave past its pass-1 rows takes variant sites from that queue and tallies
//                        mapq + ranks (+ calls) as bv_pass2_dma_kernel tallies them -- from registers, by plain loads
//                        (bv_f_p2_rows; the solver waves too, once they are out of jobs), or with BV_FLAG_P2_TAIL_DMA through the
//                        ring (again four 1 KiB pieces per slot: the counted waits are unchanged).  The solvers' last jobs
//                        run UNDER these rows, and pass 2 has no launch, fill or drain of its own.
//   no row to stream     a streaming wave whose ring is idle (waiting for a variant row, or done) solves with the ring as
//                        scratch; only such waves (12 KiB each) take the candidates that need the wave solver of bv_solver.h
//                        (shallow sites, phred-0 calls, more than 128 bins).
//
// Hand-off.  A row's summary and bins go to HBM scratch as before; they are PUBLISHED (queue entry / the wave's `pub` mark in
// LDS) one row later, behind an s_waitcnt that covers exactly the stores of that row (vmcnt counts in issue order), and read
// by the solvers through the L2 (sc1 loads; summaries of neighbouring sites share lines).  Producer and consumer are waves
// of one CU: one L2, no cross-XCD visibility involved.  Streaming waves never wait for solver waves except on a full queue,
// and every such wait is bounded (BV_F_SPIN_MAX -> BV_CTR_TIMEOUT: a loud failure, not a hung GPU).
//
// Two register allocations.  The streaming loop (bv_f_stream_until_idle) and the row re-do (bv_f_p2_redo) are functions of
// their own, NOT inlined: see the comment at the first.  The solver step has one call site for both kinds of waves.
//
// Reference functions realised: those of bv_pass1_short.hip and bv_pass2_dma_kernel (src/basetype.cpp:22-295,
// src/algorithm.h:44-255, htslib/kfunc.c:39-143,197-313; rank sums: src/basetype.cpp:201-242 via caller.cpp:1151-1154); every
// record is byte-identical to the three-launch form's (same bins, same order, same solver code).  HBM-bound by design
// (2 B per cell of every row + 4 B per cell of a variant row, the call byte of a variant row read twice); no MFMA
// (categorical tallies).  Measurements, rejected variants: DESIGN.md section 4.3.
#define BV_LNFACT_TABLE_ONLY 1  /* rows of at most 65,535 samples: see bv_lnfact */
#include "bv_kernels.h"

#include "bv_solver.h"
#include "bv_solver16.h"
#include "bv_tally.h"

#include "bv_short.h"
#include "bv_pass2_sweep.h"

#include <type_traits>

#include "bv_fused_shared.h"
#include "bv_fused_lds.h"
#include "bv_fused_solver.h"
#include "bv_fused_stream.h"
#include "bv_fused_p2rows.h"

template <bool FUSE2>
__global__ __launch_bounds__(BV_WAVE *BV_F_NW) void bv_p1s_fused_kernel(BvP1ShortArgs a) {
    __shared__ BvFusedShared sh;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // every workgroup owns a contiguous range of sites
    const uint32_t B0 = (uint32_t)((uint64_t)a.n_sites * blockIdx.x / gridDim.x), B1 = (uint32_t)((uint64_t)a.n_sites * (blockIdx.x + 1) / gridDim.x);
    // ---- set-up: histograms zeroed, queues empty, tables in LDS; nothing is in flight yet, so a plain barrier is fine
    if (wave < BV_F_NS) {
        uint4 *h4 = reinterpret_cast<uint4 *>(sh.hist[wave]);
#pragma unroll
        for (int i = 0; i < (BV_S_HWORDS + BV_S_OVF + 8) / 4 / BV_WAVE + 1; ++i)
            if (i * BV_WAVE + lane < (BV_S_HWORDS + BV_S_OVF + 8) / 4) h4[i * BV_WAVE + lane] = make_uint4(0, 0, 0, 0);
    }
    for (int i = tid; i < BV_F_QCAP; i += BV_WAVE * BV_F_NW) { sh.q3[i] = BV_F_EMPTY; sh.q2[i] = BV_F_EMPTY; }
    for (int i = tid; i < BV_F_QVCAP; i += BV_WAVE * BV_F_NW) sh.qv[i][0] = BV_F_EMPTY;
    for (int i = tid; i < BV_QBINS; i += BV_WAVE * BV_F_NW) {
        sh.tab_hit[i] = a.tables->hit[i];
        sh.tab_miss[i] = a.tables->miss[i];
        sh.tab_loghit[i] = a.tables->loghit[i];
        sh.tab_logmiss[i] = a.tables->logmiss[i];
    }
    if (tid < 16) sh.ctl[tid] = 0u;
    if (tid < BV_F_NS) sh.pub[tid] = B0;
#ifdef BV_TEAM_DEBUG
    if (tid == 0) {
        uint32_t *dbg_ = a.counters + BV_CTR_WORDS + (blockIdx.x < 512u ? blockIdx.x : 511u) * 8u;
        dbg_[0] = (uint32_t)__builtin_amdgcn_s_memrealtime(); dbg_[3] = 0u; dbg_[5] = 0u;
        dbg_[7] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
        if (blockIdx.x == 0) a.counters[BV_CTR_WORDS + 5150] = 4u;  // whose stamps these are
#ifdef BV_PHASE_DEBUG
        if (blockIdx.x == 0) for (int i = 0; i < 60; ++i) a.counters[BV_CTR_WORDS + 4200 + i] = 0u;
#endif
    }
#endif
    __syncthreads();

    const bool is_stream = wave < BV_F_NS;
    bool streaming = is_stream;
    uint32_t sst = 0;
    BvFusedSolver v;
    v.sa.ref_base = a.ref_base; v.sa.out = a.out; v.sa.var_list = a.var_list; v.sa.counters = a.counters;
    v.sa.min_af = a.min_af; v.sa.flags = a.flags;
    {
        // (wave-uniform values read through vector loads -- the tables are not provably unwritten -- go to scalar registers:
        // as vector registers they are live across the whole loop and end up in scratch memory)
        const uint64_t lf = (uint64_t)(uintptr_t)a.tables->lnfact;
        v.sa.lnfact.t = (decltype(v.sa.lnfact.t))(uintptr_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(lf >> 32)) << 32) |
                                                           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)lf));
        v.sa.lnfact.n = __builtin_amdgcn_readfirstlane((int)a.tables->lnfact_n);
    }
    v.sa.loghit = a.tables->loghit; v.sa.logmiss = a.tables->logmiss;
    v.sa.bs = a.bs; v.sa.q = a.q; v.sa.pitch = a.pitch; v.sa.n_samples = a.n_samples;
    v.n_vl = 0;
    v.fuse2 = FUSE2;
    // this wave's solver scratch: a streaming wave's ring (while no row is in flight), a solver wave's own
    if (is_stream) {
        v.grp = &sh.ring[wave].solve.ws.grp[0][0]; v.vl = sh.ring[wave].solve.vl; v.big = &sh.ring[wave].solve.ws;
    } else {
        v.grp = &sh.grp[wave - BV_F_NS][0][0]; v.vl = sh.vl[wave - BV_F_NS]; v.big = nullptr;
    }
    const uint32_t sh_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) BvFusedShared *)&sh;
    const uint64_t ka_ptr = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();  // the argument block `a`, as the streaming function reads it
    // A streaming wave streams while it has rows; whenever none is in flight (waiting for a variant row, or finished) it does
    // one unit of solver work with its ring as scratch.  ONE call site of the solver step for both kinds of waves (the solver
    // is most of the kernel's code).
#pragma unroll 1
    for (;;) {
        // A streaming wave past its pass-1 rows calls the streaming function only when a variant row waits (two LDS words
        // tell): until round 5 the function's prologue saved 60 callee-saved VGPRs to scratch memory per call, and waves that
        // polled through it wrote 316 MB per launch of 8,192 sites.  The saves are gone (see the function), the test stays: a
        // call still reads the argument block and sets the ring up.
        // (the tagged rank layout only: with the call plane to read as well the plain loads lose to the ring -- 0.533 against 0.519 ms)
        const bool p2_regs = FUSE2 && a.rpr_tag != 0u && !(a.flags & BV_FLAG_P2_TAIL_DMA);
        bool go = streaming;
        if (streaming && (sst & BV_FS_CUR_DONE) && (sst & BV_FS_P1_FIN)) {
            if (!FUSE2) { go = false; streaming = false; }
            else if (bv_f_lds_read_u(&sh.ctl[BV_FC_QV_TAIL]) == bv_f_lds_read_u(&sh.ctl[BV_FC_QV_HEAD]) &&
                     bv_f_lds_read_u(&sh.ctl[BV_FC_OV_TAIL]) == bv_f_lds_read_u(&sh.ctl[BV_FC_OV_HEAD])) {
                go = false;
                if (bv_f_no_row_ever(sh.ctl)) streaming = false;
            }
        }
        // (the lane number as a value the compiler cannot see through: what the solver derives from it -- lane & 15, masks,
        // scratch offsets, some forty values -- was hoisted out of this loop and then lived in scratch memory, a memory trip per use)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        if (go) {
            // (the wave's variant sites since its last flush sit in its ring's LDS: out before rows stream through it again)
            if (v.n_vl) bv_p1s_flush_vl(a, v.vl, v.n_vl, ln);
            // past its pass-1 rows a wave tallies the variant sites' rows from registers (bv_f_p2_rows); until then -- and with
            // BV_FLAG_P2_TAIL_DMA always -- rows go through the ring
            if (p2_regs && (sst & BV_FS_CUR_DONE) && (sst & BV_FS_P1_FIN)) {
                // Candidates first.  Behind the last pass-1 row the launch is as long as the solver's last jobs (62-74 us each) plus the rows
                // of the variant sites they find; a candidate that waits for a solver wave to finish its job first adds up to a whole
                // job to that -- and keeps the solver waves from joining the tally of the rows.
                const uint32_t least = bv_f_lds_read_u(&sh.ctl[BV_FC_NDONE]) == (uint32_t)BV_F_NS ? 1u : BV_F_MIN_JOB;
                const bool cand = bv_f_lds_read_u(&sh.ctl[BV_FC_Q3_TAIL]) - bv_f_lds_read_u(&sh.ctl[BV_FC_Q3_HEAD]) >= least ||
                                  bv_f_lds_read_u(&sh.ctl[BV_FC_Q2_TAIL]) - bv_f_lds_read_u(&sh.ctl[BV_FC_Q2_HEAD]) >= least;
                if (!cand) bv_f_p2_rows((uint32_t)ka_ptr, (uint32_t)(ka_ptr >> 32), sh_lds, (uint32_t)(uintptr_t)(bv_lds_u32 *)sh.hist[wave], B0);
            } else if (FUSE2 && !((sst & BV_FS_CUR_DONE) && (sst & BV_FS_P1_FIN)))
                // (until a wave is past its pass-1 rows its ring carries nothing else, whatever streams the variant rows later: the
                // instance of the function without the pass-2 tally -- it returns when the cursor is exhausted and its rows are out)
                sst = (uint32_t)__builtin_amdgcn_readfirstlane((int)bv_f_stream_until_idle<FUSE2, false>((uint32_t)ka_ptr, (uint32_t)(ka_ptr >> 32), sh_lds, (uint32_t)wave, B0, B1, sst));
            else
                sst = (uint32_t)__builtin_amdgcn_readfirstlane((int)bv_f_stream_until_idle<FUSE2, FUSE2>((uint32_t)ka_ptr, (uint32_t)(ka_ptr >> 32), sh_lds, (uint32_t)wave, B0, B1, sst));
            if (sst & BV_FS_P_DONE) streaming = false;
        }
        const int r = bv_f_solver_step(a, sh, v, B0, B1, ln);
        if (streaming) {
            if (r != 1) __builtin_amdgcn_s_sleep(8);
            continue;
        }
        if (p2_regs && !is_stream && r != 1) {
            // A solver wave with nothing to solve: once every streaming wave is past its pass-1 rows it tallies variant rows too -- from
            // registers, with its group scratch as the histogram (zeroed here, and left zero) -- and stays until no row can come any more.
            if (bv_f_lds_read_u(&sh.ctl[BV_FC_NDONE]) == (uint32_t)BV_F_NS) {
                if (bv_f_lds_read_u(&sh.ctl[BV_FC_QV_TAIL]) != bv_f_lds_read_u(&sh.ctl[BV_FC_QV_HEAD]) ||
                    bv_f_lds_read_u(&sh.ctl[BV_FC_OV_TAIL]) != bv_f_lds_read_u(&sh.ctl[BV_FC_OV_HEAD])) {
                    if (v.n_vl) bv_p1s_flush_vl(a, v.vl, v.n_vl, ln);
                    bv_p1s_zero_hist<false>(v.grp, ln);
                    bv_lrt_sync<0>();
                    bv_f_p2_rows((uint32_t)ka_ptr, (uint32_t)(ka_ptr >> 32), sh_lds, (uint32_t)(uintptr_t)(bv_lds_u32 *)v.grp, B0);
                    continue;
                }
                if (r == 2 && bv_f_no_row_ever(sh.ctl)) break;
            }
            __builtin_amdgcn_s_sleep(8);
            continue;
        }
        if (r == 2) break;
        if (r == 0) __builtin_amdgcn_s_sleep(8);
    }
    // (the solver step that reports "nothing left, ever" has flushed the wave's variant list)
#ifdef BV_TEAM_DEBUG
    if (lane == 0) atomicMax(&a.counters[BV_CTR_WORDS + (blockIdx.x < 512u ? blockIdx.x : 511u) * 8u + 3u], (uint32_t)__builtin_amdgcn_s_memrealtime());
#endif
}

// ------------------------------------------------------------------------------ launcher
bool bv_p1s_fused_takes(const BvP1ShortArgs &a) {
    // rows of at least BV_F_K slots (the prefetch then never runs more than one row ahead); chained launches too (the planes of
    // a row are looked up per segment where its address is formed; ref_base / out are the engine's contiguous copies)
    const uint32_t n_chunks = (a.n_samples + 15u) >> 4, n_slots = (n_chunks + 127u) >> 7;
    return n_slots >= (uint32_t)BV_F_K && a.n_samples <= BV_SHORT_ROW_MAX;
}
void bv_launch_p1s_fused(const BvP1ShortArgs &a, hipStream_t stream) {
    const uint32_t cu = a.n_cu ? a.n_cu : 256u;
    uint32_t grid = cu;
    const uint32_t need = (a.n_sites + BV_F_NS - 1) / BV_F_NS;  // at least one site per streaming wave
    if (grid > need) grid = need > 0 ? need : 1;
    const uint32_t cap = (a.flags >> 16) & 0xFFu;  // BV_FLAG_GRID_LIMIT
    if (cap && grid > cap) grid = cap;
    // with the rank planes (a.mapq, a.rpr): the variant sites' pass-2 rows are streamed by the same waves
    if (a.mapq != nullptr && a.rpr != nullptr) hipLaunchKernelGGL(bv_p1s_fused_kernel<true>, dim3(grid), dim3(BV_WAVE * BV_F_NW), 0, stream, a);
    else hipLaunchKernelGGL(bv_p1s_fused_kernel<false>, dim3(grid), dim3(BV_WAVE * BV_F_NW), 0, stream, a);
}
