// bv_fused_stream.h -- the streaming side of the fused short-row kernel: publishing pass-1 rows to the solvers, the window-sweep
// re-do of a long-read row (bv_f_p2_redo), the stash of rank sums, the argument block and a site's planes as the non-inlined functions
// read them (bv_f_args, bv_f_planes), and the streaming loop itself (bv_f_stream_until_idle).
// Included by bv_pass1_fused.hip alone, behind bv_fused_shared.h and bv_fused_lds.h; bv_fused_p2rows.h uses its stash, re-do,
// bv_f_args and bv_f_planes.
#pragma once

// ------------------------------------------------------------------------------ the streaming side
// "No variant row will ever come again" (FUSE2), read in THIS order: (1) every streaming wave has published its last pass-1
// row -- the candidate queues only shrink from here on; (2) the candidate queues are empty -- whoever took their last entries
// had counted itself in BUSY before it claimed them (bv_f_solver_step); (3) no job is counted -- those jobs are over, and a job
// pushes its variant sites before it leaves the count; (4) the variant queue is empty -- nothing can refill it.  (BUSY read
// before the queues would leave a window: BUSY == 0, then a solver counts itself and claims the last entries, then the queues
// and the variant queue are all seen empty while that job's variant rows are still to come.)
__device__ __forceinline__ bool bv_f_no_row_ever(const uint32_t *ctl) {
    if (bv_f_lds_read_u(&ctl[BV_FC_NDONE]) != (uint32_t)BV_F_NS) return false;
    if (bv_f_lds_read_u(&ctl[BV_FC_Q3_TAIL]) != bv_f_lds_read_u(&ctl[BV_FC_Q3_HEAD]) ||
        bv_f_lds_read_u(&ctl[BV_FC_Q2_TAIL]) != bv_f_lds_read_u(&ctl[BV_FC_Q2_HEAD]) ||
        bv_f_lds_read_u(&ctl[BV_FC_QH_TAIL]) != bv_f_lds_read_u(&ctl[BV_FC_QH_HEAD]))
        return false;
    if (bv_f_lds_read_u(&ctl[BV_FC_BUSY]) != 0u) return false;
    return bv_f_lds_read_u(&ctl[BV_FC_QV_TAIL]) == bv_f_lds_read_u(&ctl[BV_FC_QV_HEAD]) &&
           bv_f_lds_read_u(&ctl[BV_FC_OV_TAIL]) == bv_f_lds_read_u(&ctl[BV_FC_OV_HEAD]);
}
typedef volatile __attribute__((address_space(3))) uint32_t bv_lds_vu32;
__device__ __forceinline__ void bv_f_push(bv_lds_vu32 *q, bv_lds_u32 *tail, uint32_t site, uint32_t *counters, bool lose_first, int lane) {
    const uint32_t pos = bv_lds_fetch_add_wave((uint32_t)(uintptr_t)tail, 1u);
    bv_lds_vu32 *e = q + (pos & (BV_F_QCAP - 1u));
    // (a slot still occupied: the solvers are BV_F_QCAP candidates behind -- they never wait for a streaming wave, so this ends)
    uint32_t spins = 0;
    while ((uint32_t)__builtin_amdgcn_readfirstlane((int)*e) != BV_F_EMPTY && spins < BV_F_SPIN_MAX) { __builtin_amdgcn_s_sleep(8); ++spins; }
    if (spins == BV_F_SPIN_MAX) {
        // gave up: the entry that sits there is not overwritten (its consumer may still come), this site is not solved, and the
        // submit fails loudly (the consumer of position `pos` times out in its turn)
        if (lane == 0) atomicOr(&counters[BV_CTR_TIMEOUT], BV_TMO_PUSH);  // (OR, not add: repeated events must not carry into the next field, or wrap the word to 0)
        return;
    }
    // (BV_FLAG_FAULT_LOST_HANDOFF, tests: the first entry of every workgroup's queue is reserved and never written -- the solver
    // wave that claims it must give up after its bounded wait)
    if (lose_first && pos == 0u) return;
    if (lane == 0) *e = site;
}
// publish a pass-1 row whose stores are complete.  Candidates of the 16-lane solver: a place in their queue -- one LDS atomic,
// one LDS write (the slot is free once its last consumer has handed it back empty).  Candidates of the wave solver: a place in
// the workgroup's slice of cand_list in HBM (unbounded: they are taken up only when every streaming wave is past its last
// pass-1 row, see bv_f_solver_step, so no streaming wave ever waits on them); that store is one more in the vmcnt queue than
// the slot waits allow for -- a conservative wait, never a wrong one.
__device__ __forceinline__ void bv_f_publish(const BvP1ShortArgs &a, BvFusedShared &sh, uint32_t B0, uint32_t site, uint32_t kind, int lane) {
    if (kind < 2u) return;
    if (kind == 4u) {
        const uint32_t pos = bv_lds_fetch_add_wave((uint32_t)(uintptr_t)(bv_lds_u32 *)&sh.ctl[BV_FC_QH_TAIL], 1u);
        if (lane == 0) a.cand_list[B0 + pos] = site;  // (a slot per site of the workgroup's range: the list cannot outgrow them)
    } else if (kind == 3u) {
        bv_f_push((bv_lds_vu32 *)sh.q3, (bv_lds_u32 *)&sh.ctl[BV_FC_Q3_TAIL], site, a.counters, (a.flags & BV_FLAG_FAULT_LOST_HANDOFF) != 0u, lane);
    } else {
        bv_f_push((bv_lds_vu32 *)sh.q2, (bv_lds_u32 *)&sh.ctl[BV_FC_Q2_TAIL], site, a.counters, (a.flags & BV_FLAG_FAULT_LOST_HANDOFF) != 0u, lane);
    }
}
// A variant row with a read-position rank beyond the 256-rank window of the fast tally (long reads): the exact re-do of
// bv_pass2_sweep.h (bv_p2_wave_exact) -- plain loads, as bv_pass2_dma_kernel falls back to it -- into the wave's histogram, the two
// rank sums stored at once.  Rare, and not inlined: the streaming loop keeps its registers; the loads' waits drain the ring.
__device__ __attribute__((noinline)) void bv_f_p2_redo(const uint8_t *bs_, const uint8_t *mapq_, const uint16_t *rpr_, bv_site_result *out_, uint64_t pitch,
                                                       uint32_t n_samples, uint32_t site_, uint32_t lut_, uint32_t n12_, uint32_t hist_lds_) {
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t site = (uint32_t)__builtin_amdgcn_readfirstlane((int)site_), lut_tag = (uint32_t)__builtin_amdgcn_readfirstlane((int)lut_);
    const uint32_t lut = lut_tag & 0xFFu;  // bit 31: the rank plane is tagged (BV_SLAB_RPR_TAGGED)
    const uint32_t n12 = (uint32_t)__builtin_amdgcn_readfirstlane((int)n12_);
    uint32_t *h = (uint32_t *)(bv_lds_u32 *)(uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)hist_lds_);
    bv_site_result *out = (bv_site_result *)(__attribute__((address_space(1))) bv_site_result *)out_;
    BvPass2Args as;
    as.bs = (const uint8_t *)(__attribute__((address_space(1))) const uint8_t *)bs_;
    as.mapq = (const uint8_t *)(__attribute__((address_space(1))) const uint8_t *)mapq_;
    as.rpr = (const uint16_t *)(__attribute__((address_space(1))) const uint16_t *)rpr_;
    as.q = nullptr; as.group_id = nullptr; as.pitch = pitch; as.n_samples = n_samples; as.n_groups = 0;
    const unsigned long long n1 = n12 & 0xFFFFu, n2 = n12 >> 16;
    bv_p2_wave_exact<256>(as, out, site, lut, bv_rpr_rank_mask(lut_tag >> 31), n1, n2, h, h + 512, lane);
    bv_lrt_sync<0>();
}

// pass-2 results of up to 64 rows of one wave, one row per lane: the two rank sums as exact integers, turned into phred values
// (erfc, log10: scalar work per site) and stored for all of them at once
struct BvFusedStash {
    uint32_t site, n12;
    unsigned long long tw_m, tw_r;
    uint32_t n;  // rows held (wave-uniform)
};
__device__ __forceinline__ void bv_f_stash_flush(const BvP1ShortArgs &a, BvFusedStash &t, int lane) {
    if ((uint32_t)lane < t.n) {
        const unsigned long long n1 = t.n12 & 0xFFFFu, n2 = t.n12 >> 16;
        const double ph_m = bv_ranksum_phred(t.tw_m, n1, n2), ph_r = bv_ranksum_phred(t.tw_r, n1, n2);
        a.out[t.site].mq_ranksum = ph_m;
        a.out[t.site].rpr_ranksum = ph_r;
        atomicOr(&a.out[t.site].status, BV_SITE_RANKSUM);
    }
    t.n = 0;
}

// Streams rows until none is in flight and none can be drawn right now.  `st_io`: the wave's flags that outlive a call (cursor
// exhausted / last pass-1 row published / no row will ever come again).  On return the ring is idle (it can serve as solver
// scratch), no pass-1 row of this wave is unpublished and the pass-2 results of its rows are stored.
//
// NOT inlined.  Inlined into the kernel's loop beside the solver (which wants all of its 168 registers), the allocator parked
// this loop's lane constants in scratch memory: a scratch load behind an s_waitcnt vmcnt(0) -- a drained ring -- per row.  As a
// function of its own it has a register allocation of its own.  What it needs arrives so that everything stays what it is in
// a kernel: the argument block is read from the kernel's own kernarg segment (scalar loads, wave-uniform by construction; its
// pointers are marked as device memory), the LDS block comes as an LDS ADDRESS and is turned back into a pointer here (a generic
// pointer handed across a call would make every access a flat one), the lane number is formed here.
// not_tail_called: clang marks the kernel's call `tail`, and a function with a tail-marked caller keeps the callee-saved
// registers of the AMDGPU convention -- its prologue stored the 60 of them it uses (v40-47, v56-63, ...) to scratch memory,
// 15 KB per wave and call, and the L2 wrote 85 MB of that back per launch.  Without the mark LLVM's inter-procedural register
// allocation applies to this local, non-recursive function: no saves here, the kernel keeps what IT has live across the call
// (next to nothing: see the lane number in the kernel's loop).
#define BV_F_GLOBAL(T, p) ((T *)(__attribute__((address_space(1))) T *)(p))
// the argument block as the non-inlined functions read it back (fields a caller does not use cost it nothing)
__device__ __forceinline__ BvP1ShortArgs bv_f_args(uint32_t ka_lo_, uint32_t ka_hi_) {
    BvP1ShortArgs a;
    // (the kernel hands its kernarg segment pointer over: the intrinsic itself read null in this function)
    const uint64_t kp = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)ka_hi_) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)ka_lo_);
    const __attribute__((address_space(4))) BvP1ShortArgs *ka = (const __attribute__((address_space(4))) BvP1ShortArgs *)(uintptr_t)kp;
    a.bs = BV_F_GLOBAL(const uint8_t, ka->bs); a.q = BV_F_GLOBAL(const uint8_t, ka->q); a.ref_base = BV_F_GLOBAL(const uint8_t, ka->ref_base);
    a.pitch = ka->pitch; a.n_sites = ka->n_sites; a.n_samples = ka->n_samples; a.flags = ka->flags; a.n_cu = ka->n_cu;
    a.min_af = ka->min_af; a.tables = BV_F_GLOBAL(const BvTables, ka->tables); a.out = BV_F_GLOBAL(bv_site_result, ka->out);
    a.var_list = BV_F_GLOBAL(uint32_t, ka->var_list); a.counters = BV_F_GLOBAL(uint32_t, ka->counters);
    a.summ = BV_F_GLOBAL(BvSiteSummary, ka->summ); a.bins = BV_F_GLOBAL(uint32_t, ka->bins);
    a.cand_list = BV_F_GLOBAL(uint32_t, ka->cand_list); a.easy_list = BV_F_GLOBAL(uint32_t, ka->easy_list);
    a.easy3_list = BV_F_GLOBAL(uint32_t, ka->easy3_list); a.ch = BV_F_GLOBAL(const BvChain, ka->ch);
    a.mapq = BV_F_GLOBAL(const uint8_t, ka->mapq); a.rpr = BV_F_GLOBAL(const uint16_t, ka->rpr);
    a.ovf = BV_F_GLOBAL(uint32_t, ka->ovf);
    a.rpr_tag = ka->rpr_tag;
    return a;
}
// The planes that hold a site's rows.  A chained launch: those of the segment that holds the site, biased so that the global site
// number indexes them -- read through the constant address space: scalar loads, outside the counted vmcnt queue.
struct BvFusedPlanes {
    const uint8_t *bs, *q, *mq;
    const uint16_t *rp;
};
__device__ __forceinline__ BvFusedPlanes bv_f_planes(const BvP1ShortArgs &a, uint32_t site) {
    BvFusedPlanes p = {a.bs, a.q, a.mapq, a.rpr};
    if (a.ch != nullptr) {
        const BvChainC ch = bv_chain_const(a.ch);
        const uint32_t sg = bv_chain_seg(ch, site);
        p.bs = ch->bs[sg]; p.q = ch->q[sg]; p.mq = ch->mapq[sg]; p.rp = ch->rpr[sg];
    }
    return p;
}
// P2RING: the ring carries the variant sites' pass-2 rows too (FUSE2 with plain ranks, or BV_FLAG_P2_TAIL_DMA); false: pass-1 rows only
// -- the instance FUSE2 launches of tagged slabs take: without the pass-2 tally in its loop it has no scalar registers spilled there.
template <bool FUSE2, bool P2RING = FUSE2>
__device__ __attribute__((noinline, not_tail_called)) uint32_t bv_f_stream_until_idle(uint32_t ka_lo_, uint32_t ka_hi_, uint32_t sh_lds_, uint32_t wave_, uint32_t B0_,
                                                                     uint32_t B1_, uint32_t st_in_) {
    const uint32_t sh_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh_lds_);
    const int wave = __builtin_amdgcn_readfirstlane((int)wave_);
    const uint32_t B0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)B0_), B1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)B1_);
    uint32_t st_io = (uint32_t)__builtin_amdgcn_readfirstlane((int)st_in_);
    BvFusedShared &sh = *(BvFusedShared *)(__attribute__((address_space(3))) BvFusedShared *)(uintptr_t)sh_lds;
    const BvP1ShortArgs a = bv_f_args(ka_lo_, ka_hi_);
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    uint32_t *hist = sh.hist[wave];
    uint32_t *stage = sh.stage[wave];
    const uint32_t ring_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(bv_lds_u32 *)sh.ring[wave].slot[0]);
    const uint32_t *ring = sh.ring[wave].slot[0];
    const uint32_t cursor_lds = (uint32_t)(uintptr_t)(bv_lds_u32 *)&sh.ctl[BV_FC_CURSOR];
    const uint32_t qvhead_lds = (uint32_t)(uintptr_t)(bv_lds_u32 *)&sh.ctl[BV_FC_QV_HEAD];
    const uint32_t ovhead_lds = (uint32_t)(uintptr_t)(bv_lds_u32 *)&sh.ctl[BV_FC_OV_HEAD];
    // ---- the geometry of a row (the same for every row of a kind)
    const uint32_t n_chunks = (a.n_samples + 15u) >> 4;  // 16-byte chunks of a plane's row
    const int tail = (int)(a.n_samples & 15u);
    // pass-1 rows: slots of 128 chunks (2 KiB of calls + 2 KiB of phreds)
    const uint32_t n_slots1 = (n_chunks + 127u) >> 7;
    const uint32_t last1 = n_chunks - (n_slots1 - 1u) * 128u;  // chunks of a row's last slot that lie inside the row: 1 .. 128
    const uint32_t va = (uint32_t)lane * 16u, vb = va + 1024u;
    const uint32_t vbl = last1 > 64u ? vb : va;
    const unsigned long long mA1 = last1 >= 64u ? ~0ull : ((1ull << last1) - 1ull);
    const unsigned long long mB1 = last1 > 64u ? (last1 >= 128u ? ~0ull : ((1ull << (last1 - 64u)) - 1ull)) : 1ull;
    // pass-2 rows: slots of 64 chunks (1 KiB of calls, 1 KiB of mapq, 2 KiB of ranks: 32 bytes per lane in two pieces)
    const uint32_t n_slots2 = (n_chunks + 63u) >> 6;
    const uint32_t last2 = n_chunks - (n_slots2 - 1u) * 64u;   // 1 .. 64
    // The 2 KiB of ranks arrive as two CONTIGUOUS KiB (lane l: bytes 16 l .. 16 l + 15 of each), not as the lane's own 32 bytes in two
    // halves: a piece of 64 x 16 bytes at a stride of 32 touches sixteen 128-byte lines instead of eight, and its twin the same
    // sixteen again -- in the launch's last phase, where only such rows stream, requesting a slot took 1,260 cycles against 420
    // for a pass-1 slot and the slot then came late (1,870 cycles of waiting per slot; round 6, -DBV_PHASE_DEBUG).  The lane's own
    // 32 bytes are put together where the slot is read: two ds_read_b128 at a stride of 32.
    const unsigned long long mA2 = last2 >= 64u ? ~0ull : ((1ull << last2) - 1ull);
    // a row's last slot: the lanes of the two rank pieces that lie inside the row (2 x last2 chunks of 16 bytes)
    const unsigned long long mR0 = last2 >= 32u ? ~0ull : ((1ull << (2u * last2)) - 1ull);
    const unsigned long long mR1 = last2 > 32u ? (last2 >= 64u ? ~0ull : ((1ull << (2u * last2 - 64u)) - 1ull)) : 1ull;
    const uint32_t vrl = last2 > 32u ? vb : va;  // (a second piece wholly past the row's end: lane 0 alone re-reads valid bytes)
    // the last slot's cells past the row's end are forced to 'N': per lane and dword, the mask of the bytes that stay
    uint32_t keepA[4], keepB[4], keep2[4];
    {
        const uint32_t cA = (uint32_t)lane, cB = 64u + (uint32_t)lane;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int partial = tail ? tail - 4 * d : 4;
            keepA[d] = cA >= last1 ? 0u : ((cA == last1 - 1u) ? bv_f_keep_mask(partial) : 0xFFFFFFFFu);
            keepB[d] = cB >= last1 ? 0u : ((cB == last1 - 1u) ? bv_f_keep_mask(partial) : 0xFFFFFFFFu);
            keep2[d] = cA >= last2 ? 0u : ((cA == last2 - 1u) ? bv_f_keep_mask(partial) : 0xFFFFFFFFu);
        }
    }
    uint32_t one;
    asm volatile("v_mov_b32 %0, 1" : "=v"(one));
    // the tagged rank layout (BV_SLAB_RPR_TAGGED): a pass-2 row is mapq + ranks, the class of a cell comes from its rank word
    const bool tag = P2RING && a.rpr_tag != 0u;
    const uint32_t hi_mask = bv_rpr_hi_mask(tag ? 1u : 0u);

    // ---- prefetch side: the next slot to request
    const uint8_t *p0 = a.bs, *p1 = a.q, *p2 = a.q;  // pass 1: calls, phreds; pass 2: calls, mapq, ranks
    uint32_t p_left = 0, p_kind = 0;    // slots of the prefetch row still to request; its kind
    uint32_t ring_w = 0, ring_r = 0, inflight = 0;
    // rows drawn: the one being tallied and the one after it (the prefetch runs at most one row ahead: every row has >= BV_F_K slots)
    // x / y: pass 1: reference base / -; pass 2: class table / n_ref | n_alt << 16; z: pass 2: the sweeps' 2-bit table
    uint32_t c_site = 0, c_kind = 0, c_x = 0, c_y = 0, c_z = 0, n_site = 0, n_kind = 0, n_x = 0, n_y = 0, n_z = 0;
    uint32_t st = st_io;
    BV_PH_DECL;
    constexpr uint32_t P_DONE = BV_FS_P_DONE, C_HAVE = 2u, N_HAVE = 4u, CUR_DONE = BV_FS_CUR_DONE, P1_FIN = BV_FS_P1_FIN;
    auto issue = [&]() __attribute__((always_inline)) {
        if (p_left == 0u) {
            if (st & P_DONE) return;
            uint32_t s = 0, kind = 0, x = 0, y = 0, z = 0;
            // the next row: a pass-1 row while the cursor has any, then the variant sites' pass-2 rows.  (Until round 6 a wave took a
            // variant row first whenever 64 of them were waiting.  Rows of the two kinds mixed cost more than the same rows one
            // kind after the other -- thresholds of 2 / 8 / 24 measured -9 / -9 / -5 % at 100,000 sites, "never" +2.5 % at 524,288,
            // where the queue does reach 64 --, and nothing needs it: a full variant queue spills to the overflow list.)
            if (!(st & CUR_DONE)) {
                const uint32_t c = bv_lds_fetch_add_wave(cursor_lds, 1u);
                if (c < B1 - B0) { s = B0 + c; kind = BV_FK_P1; x = bv_f_ref_scalar(a.ref_base, s); }
                else st |= CUR_DONE;
            }
            // (a wave past its pass-1 rows streams what variant rows there are; one that solved first instead measured 168
            // against 175 M sites/s: HBM idles while twelve waves solve)
            // (The draw -- one attempt on the queue, one on the overflow list -- stands here and in pop() of bv_f_p2_rows.  As one function
            // for both its result is decided behind a lane-0 branch, the compiler takes this loop's ring state for per-lane values
            // unless the result goes through a readfirstlane, and with that the register allocation around the two calls moved:
            // bv_p1s_fused_kernel<true> went from 5 to 60 scratch operations.  Two copies; a fix to one goes into the other.)
            if (P2RING && kind == 0u) {
                const uint32_t h = bv_f_lds_read_u(&sh.ctl[BV_FC_QV_HEAD]);
                if (h != bv_f_lds_read_u(&sh.ctl[BV_FC_QV_TAIL]) && bv_f_lds_cas_wave(qvhead_lds, h, h + 1u) == h) {
                    const uint32_t *e = sh.qv[h & (BV_F_QVCAP - 1u)];
                    for (uint32_t spins = 0; (s = bv_f_lds_read_u(&e[0])) == BV_F_EMPTY && spins < BV_F_SPIN_MAX; ++spins) __builtin_amdgcn_s_sleep(4);
                    x = bv_f_lds_read_u(&e[1]); y = bv_f_lds_read_u(&e[2]); z = bv_f_lds_read_u(&e[3]);
                    if (lane == 0) *(bv_lds_vu32 *)&e[0] = BV_F_EMPTY;
                    if (s == BV_F_EMPTY) { if (lane == 0) atomicOr(&a.counters[BV_CTR_TIMEOUT], BV_TMO_TAKE_VARIANT); }  // (timed out: no row, flagged)
                    else kind = BV_FK_P2;
                }
            }
            if (P2RING && kind == 0u) {
                // ... or from the overflow list (rare: more variant sites waiting than the LDS queue takes).  Its entries are in
                // HBM: one vector load, the ring drains
                const uint32_t oh = bv_f_lds_read_u(&sh.ctl[BV_FC_OV_HEAD]);
                if (oh != bv_f_lds_read_u(&sh.ctl[BV_FC_OV_TAIL]) && bv_f_lds_cas_wave(ovhead_lds, oh, oh + 1u) == oh) {
                    bv_u32x4 e;
                    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(e) : "v"(a.ovf + 4u * (size_t)(B0 + oh)) : "memory");
                    s = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.x); x = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.y);
                    y = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.z); z = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.w);
                    kind = BV_FK_P2;
                }
            }
            if (kind == 0u) {
                // no row right now.  None ever again: the cursor is exhausted, every streaming wave has published its last
                // pass-1 row, no candidate waits, no solver job runs (each is counted before its entries leave their
                // queue, until its variant sites are in theirs), and the variant queue is empty.
                if ((st & CUR_DONE) && (!FUSE2 || bv_f_no_row_ever(sh.ctl))) st |= P_DONE;
                return;
            }
            const uint64_t off = (uint64_t)s * a.pitch;
            const BvFusedPlanes pl = bv_f_planes(a, s);
            p0 = bv_uniform_ptr(pl.bs + off);
            if (kind == BV_FK_P1) { p1 = bv_uniform_ptr(pl.q + off); p_left = n_slots1; }
            else { p1 = bv_uniform_ptr(pl.mq + off); p2 = bv_uniform_ptr(reinterpret_cast<const uint8_t *>(pl.rp) + 2u * off); p_left = n_slots2; }
            p_kind = kind;
            if (!(st & C_HAVE)) { c_site = s; c_kind = kind; c_x = x; c_y = y; c_z = z; st |= C_HAVE; }
            else { n_site = s; n_kind = kind; n_x = x; n_y = y; n_z = z; st |= N_HAVE; }
        }
        BV_PH(10);
#ifdef BV_PHASE_DEBUG
        if (ring_w == 0u) ph_i0_ = (uint32_t)__builtin_amdgcn_s_memtime();  // (ring position 0 only: one in K slots is timed)
#endif
        const uint32_t d0 = ring_lds + ring_w * (BV_F_SLOT_WORDS * 4u);
        if (!P2RING || p_kind == BV_FK_P1) {
            if (p_left > 1u) { bv_f_glds4(d0, p0, va, p0, vb, p1, va, p1, vb); p0 += 2048; p1 += 2048; }
            else bv_f_glds4_masked(d0, p0, va, p0, vbl, p1, va, p1, vbl, mA1, mB1);
        } else if (tag) {
            if (p_left > 1u) { bv_f_glds4_tag(d0, p1, va, p2, va, vb); p1 += 1024; p2 += 2048; }
            else bv_f_glds4_m4(d0, p1, va, 1ull, p1, va, mA2, p2, va, mR0, p2, vrl, mR1);
        } else {
            if (p_left > 1u) { bv_f_glds4(d0, p0, va, p1, va, p2, va, p2, vb); p0 += 1024; p1 += 1024; p2 += 2048; }
            else bv_f_glds4_m4(d0, p0, va, mA2, p1, va, mA2, p2, va, mR0, p2, vrl, mR1);
        }
        --p_left;
        ring_w = (ring_w + 1u == (uint32_t)BV_F_K) ? 0u : ring_w + 1u;
        ++inflight;
    };

    // the previous pass-1 row of this wave: published once its stores are known to be complete
    uint32_t prev_site = 0, prev_kind = 0;  // kind 0: none; 1: not a candidate; 2 / 3: queue q2 / q3; 4: wave solver
    uint32_t wsel = 0;                      // stores of the previous row still to be allowed for in the slot waits: 0 none / unknown, 1, 3
    BvFusedStash stash;
    stash.site = 0; stash.n12 = 0; stash.tw_m = 0; stash.tw_r = 0; stash.n = 0;
    // the end of this wave's pass-1 rows: its last one published, the wave counted in NDONE
    auto finish_p1 = [&]() __attribute__((always_inline)) {
        if (prev_kind != 0u) {
            if (inflight == (uint32_t)BV_F_K) asm volatile(BV_F_W_ALL ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            bv_f_publish(a, sh, B0, prev_site, prev_kind, lane);
            if (prev_kind == 4u) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (its cand_list entry; rare)
            prev_kind = 0;
        }
        if (lane == 0) {
            sh.pub[wave] = 0xFFFFFFFFu;
#ifdef BV_TEAM_DEBUG  /* per workgroup: first / last streaming wave past its pass-1 rows, and what was left to solve then */
            const uint32_t now = (uint32_t)__builtin_amdgcn_s_memrealtime();
            uint32_t *dbg_ = a.counters + BV_CTR_WORDS + (blockIdx.x < 512u ? blockIdx.x : 511u) * 8u;
            if (atomicAdd(&sh.ctl[BV_FC_NDONE], 1u) == 0u) dbg_[1] = now;
            else if (sh.ctl[BV_FC_NDONE] == (uint32_t)BV_F_NS) {
                dbg_[2] = now;
                dbg_[4] = (sh.ctl[BV_FC_Q3_TAIL] - sh.ctl[BV_FC_Q3_HEAD]) | ((sh.ctl[BV_FC_Q2_TAIL] - sh.ctl[BV_FC_Q2_HEAD]) << 16);
                dbg_[6] = FUSE2 ? sh.ctl[BV_FC_QV_TAIL] - sh.ctl[BV_FC_QV_HEAD] : ((B1 - B0 + 63u) >> 6) - sh.ctl[BV_FC_BLK_HEAD];
            }
#else
            atomicAdd(&sh.ctl[BV_FC_NDONE], 1u);
#endif
        }
        st |= P1_FIN;
    };

#pragma unroll 1
    for (int k = 0; k < BV_F_K; ++k) issue();
    BV_PH(2);
#pragma unroll 1
    while (st & C_HAVE) {
        const uint32_t site = c_site;
        const bool is_p1 = !P2RING || c_kind == BV_FK_P1;
        const uint32_t n_slots = is_p1 ? n_slots1 : n_slots2;
        uint32_t hi_acc = 0, dom = BV_DOM_NONE;
#pragma unroll 1
        for (uint32_t j = 0; j < n_slots; ++j) {
            // The oldest slot in flight has landed once at most 8 younger loads are outstanding -- plus, for the three waits
            // that follow a pass-1 row's epilogue, that row's S stores, which are younger than the slot waited for (vmcnt
            // counts in issue order).  Unknown S, or fewer than K slots in flight: the conservative wait.
            if (inflight != (uint32_t)BV_F_K) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if (j >= (uint32_t)BV_F_K || wsel == 0u) asm volatile(BV_F_W_OLDEST ::: "memory");
            else if (wsel == 1u) asm volatile(BV_F_W_OLDEST_1 ::: "memory");
            else asm volatile(BV_F_W_OLDEST_3 ::: "memory");
            BV_PH(0); BV_PH_COUNT(7);
#ifdef BV_PHASE_DEBUG
            if (ring_r == 0u) { if (st & BV_FS_P1_FIN) { ph_i2_ += ph_t_ - ph_i0_; ++ph_n2_; } else { ph_i1_ += ph_t_ - ph_i0_; ++ph_n1_; } }  // requested -> found landed
#endif
            const uint32_t *rs = ring + ring_r * BV_F_SLOT_WORDS + lane * 4;
            // (a pass-2 slot: the lane's 16 ranks are 32 contiguous bytes of the slot's second half)
            const uint32_t *rs2 = (!P2RING || c_kind == BV_FK_P1) ? rs + 512 : rs + 512 + lane * 4;
            const uint32_t o3 = (!P2RING || c_kind == BV_FK_P1) ? 256u : 4u;
            bv_u32x4 w0 = *reinterpret_cast<const bv_u32x4 *>(rs);
            bv_u32x4 w1 = *reinterpret_cast<const bv_u32x4 *>(rs + 256);
            bv_u32x4 w2 = *reinterpret_cast<const bv_u32x4 *>(rs2);
            bv_u32x4 w3 = *reinterpret_cast<const bv_u32x4 *>(rs2 + o3);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // in registers: the slot may be refilled
            ring_r = (ring_r + 1u == (uint32_t)BV_F_K) ? 0u : ring_r + 1u;
            --inflight;
            BV_PH(1);
            issue();
            BV_PH(2);
            const uint32_t N4 = 0x08080808u;
            if (is_p1) {
                // w0 / w1: calls of the slot's first / second KiB; w2 / w3: their phreds
                if (j + 1u == n_slots) {
                    w0.x = (w0.x & keepA[0]) | (N4 & ~keepA[0]); w0.y = (w0.y & keepA[1]) | (N4 & ~keepA[1]);
                    w0.z = (w0.z & keepA[2]) | (N4 & ~keepA[2]); w0.w = (w0.w & keepA[3]) | (N4 & ~keepA[3]);
                    w1.x = (w1.x & keepB[0]) | (N4 & ~keepB[0]); w1.y = (w1.y & keepB[1]) | (N4 & ~keepB[1]);
                    w1.z = (w1.z & keepB[2]) | (N4 & ~keepB[2]); w1.w = (w1.w & keepB[3]) | (N4 & ~keepB[3]);
                    // (stale phred bytes of lanes that loaded nothing must not look like invalid input)
                    w2.x &= keepA[0]; w2.y &= keepA[1]; w2.z &= keepA[2]; w2.w &= keepA[3];
                    w3.x &= keepB[0]; w3.y &= keepB[1]; w3.z &= keepB[2]; w3.w &= keepB[3];
                }
                bv_f_tally2(w0, w2, w1, w3, hist, one);
                BV_PH(3);
            } else {
                // w0: calls; w1: mapq; w2 / w3: ranks 0-7 / 8-15 of the lane's 16 cells.  The tally of bv_pass2_dma_kernel
                // (bv_pass2.hip): class bytes by one v_perm per dword, class << 8 | value by one v_perm per cell, "< 0x200"
                // the whole predicate.
                const uint32_t L = c_x;
                uint32_t c0, c1, c2, c3;
                if (tag) {
                    // (w0 is not loaded: the cells' calls are the tags of their rank words)
                    if (j + 1u == n_slots) bv_f_p2t_last(w2, w3, lane, last2, tail);
                    bv_p2t_class16(L, w2, w3, c0, c1, c2, c3);
                } else {
                    if (j + 1u == n_slots) {
                        w0.x = (w0.x & keep2[0]) | (N4 & ~keep2[0]); w0.y = (w0.y & keep2[1]) | (N4 & ~keep2[1]);
                        w0.z = (w0.z & keep2[2]) | (N4 & ~keep2[2]); w0.w = (w0.w & keep2[3]) | (N4 & ~keep2[3]);
                        if ((uint32_t)lane >= last2) { w2 = bv_u32x4{0u, 0u, 0u, 0u}; w3 = w2; }  // (not loaded: stale bytes)
                    }
                    c0 = __builtin_amdgcn_perm(L, L, w0.x) ^ 0x80808080u; c1 = __builtin_amdgcn_perm(L, L, w0.y) ^ 0x80808080u;
                    c2 = __builtin_amdgcn_perm(L, L, w0.z) ^ 0x80808080u; c3 = __builtin_amdgcn_perm(L, L, w0.w) ^ 0x80808080u;
                }
                {
                // ranks that do not fit the 256-rank window: remembered, the row is then re-done by the window sweeps
                hi_acc |= (w2.x | w2.y | w2.z | w2.w | w3.x | w3.y | w3.z | w3.w) & hi_mask;
                uint32_t x[16], y[16];
                bv_p2d_xy16(c0, c1, c2, c3, w1, w2, w3, x, y);
                bv_p2d_add16(x, y, hist, hist + 512, one, ((c_y & 0xFFFFu) + (c_y >> 16)) * 8u >= a.n_samples && !(a.flags & BV_FLAG_NO_DOM), dom);
                }
                BV_PH(4);
            }
        }
        bv_lrt_sync<0>();

        // ---- the previous pass-1 row's stores are older than the (at most) K slots in flight: wait for exactly them, publish it
        if (prev_kind != 0u) {
            if (inflight == (uint32_t)BV_F_K) asm volatile(BV_F_W_ALL ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            bv_f_publish(a, sh, B0, prev_site, prev_kind, lane);
            prev_kind = 0;
            // every pass-1 row of this wave below its next one is out: the row of this epilogue, or the one already drawn, or
            // -- none drawn -- whatever the cursor hands out next (the end of the pass-1 rows sets the mark to "all")
            // (a cursor past the workgroup's own range: everything of that range this wave had is out)
            const uint32_t cur_now = bv_f_lds_read_u(&sh.ctl[BV_FC_CURSOR]);
            uint32_t mark = is_p1 ? site : (((st & N_HAVE) && n_kind == BV_FK_P1) ? n_site : (cur_now < B1 - B0 ? B0 + cur_now : 0xFFFFFFF0u));
            if (lane == 0 && !(st & P1_FIN)) sh.pub[wave] = mark;
        }

        if (is_p1) {
        // ---- the row's totals (LDS operations of one wave execute in order: the adds above are done)
        uint32_t c[4][2], facc[4], racc[4];
        bool bad = false;
        uint32_t q0_mask = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
#pragma unroll
            for (int qr = 0; qr < 2; ++qr) {
                const int q = (qr << 6) | lane;
                const uint32_t f = hist[(b << 7) | q], r = hist[((b | 4) << 7) | q];
                c[b][qr] = f + r;
                if (qr == 0) { facc[b] = f; racc[b] = r; } else { facc[b] += f; racc[b] += r; }
                if (qr == 1) bad |= (c[b][qr] != 0u) && (q >= BV_NQ_VALID);
            }
            if (__builtin_amdgcn_readfirstlane((int)c[b][0]) != 0) q0_mask |= 1u << b;
        }
        uint32_t fwd[4], rev[4];
        {
            const uint32_t vv[8] = {facc[0], facc[1], facc[2], facc[3], racc[0], racc[1], racc[2], racc[3]};
            uint32_t t[8];
            bv_wave_sum8_u32(vv, t, lane);
#pragma unroll
            for (int b = 0; b < 4; ++b) { fwd[b] = t[b]; rev[b] = t[4 + b]; }
        }
        uint32_t badq = (__ballot(bad) != 0ull) ? 1u : 0u;
        {
            uint32_t ovf_any = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t of = hist[BV_S_HWORDS + b], orv = hist[BV_S_HWORDS + 4 + b];
                fwd[b] += of; rev[b] += orv;
                ovf_any |= of | orv;
            }
            if (ovf_any) badq = 1u;
        }
        uint32_t depth[4], total = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) { depth[b] = fwd[b] + rev[b]; total += depth[b]; }

        // ---- candidate or not (as bv_p1s_stream_kernel): not a candidate = nothing covered, or exactly one active base
        // (basetype.cpp:135-139), it is the reference base, none of its calls has phred 0, and the all-sites strand table is shallow
        bool is_cand = false;
        uint32_t n_active = 0;
        if (total != 0u && !(a.flags & BV_FLAG_TALLY_ONLY)) {
            const int bsel = lane & 3;
            const bool act = (double)bv_sel4u(depth, bsel) / (int)total >= a.min_af;  // basetype.cpp:137, one base per lane
            const uint32_t act_mask = (uint32_t)(__ballot(act) & 0xFull);
            n_active = (uint32_t)__popc(act_mask);
            int ref = (int)c_x;
            if (ref > 4) ref = 4;
            const bool one_ref = act_mask != 0u && (act_mask & (act_mask - 1u)) == 0u && ref < 4 && act_mask == (1u << ref);
            is_cand = !one_ref || (q0_mask & act_mask) != 0u;
            if (!is_cand) {
                // Fisher tables of (ref_fwd, ref_rev, alt_fwd, alt_rev): imax - imin + 1 (kfunc.c:253-257)
                const uint32_t rf = bv_sel4u(fwd, ref), rr = bv_sel4u(rev, ref);
                const uint32_t af = fwd[0] + fwd[1] + fwd[2] + fwd[3] - rf;
                const int n1_ = (int)(rf + rr), n_1 = (int)(rf + af), n = (int)total;
                const int imax = n_1 < n1_ ? n_1 : n1_;
                int imin = n1_ + n_1 - n;
                if (imin < 0) imin = 0;
                is_cand = (imax - imin + 1) > BV_S_SIMPLE_MAX_TABLES;
            }
        }
        uint32_t nb = 0, kind = 1u, n_stores = 1u;
        if (is_cand) {
            // every non-empty (base, phred < 128) bin, in (base, phred) order -- the order of bv_prologue_wave
            unsigned long long m[8];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
#pragma unroll
                for (int qr = 0; qr < 2; ++qr) {
                    m[b * 2 + qr] = __ballot(c[b][qr] != 0u);
                    nb += (uint32_t)__popcll(m[b * 2 + qr]);
                }
            }
            // four per wave (bv_solver16.h) unless the site needs what only the wave solver has: the ordered replay of a
            // shallow site, the literal 0/0 arithmetic of phred-0 calls or of min_af <= 0, or more than 128 bins
            const bool is_easy = q0_mask == 0u && total > (uint32_t)BV_ORD_MAX && nb <= (uint32_t)BV_G16_MAX_BINS && a.min_af > 0.0 &&
                                 !(a.flags & BV_FLAG_WAVE_SOLVER);
            kind = is_easy ? (n_active <= 2u ? 2u : 3u) : 4u;
            uint32_t *dst = a.bins + (size_t)site * BV_S_BIN_STRIDE;
            uint32_t pos0 = 0;
            // (opaque to the optimiser: it would otherwise keep the eight bin codes of a lane as loop invariants -- in scratch
            // memory, with a scratch load and an s_waitcnt vmcnt(0), a drained ring, per candidate row)
            uint32_t lane16 = (uint32_t)lane << 16;
            asm volatile("" : "+v"(lane16));
            if (is_easy) {
                // through the LDS stage: two 64-lane stores whatever the number of bins (words past it are never read)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
#pragma unroll
                    for (int qr = 0; qr < 2; ++qr) {
                        const unsigned long long mm = m[b * 2 + qr];
                        const uint32_t pos = pos0 + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
                        if (c[b][qr] != 0u) stage[pos] = ((((uint32_t)b << 7) | ((uint32_t)qr << 6)) << 16) | lane16 | c[b][qr];
                        pos0 += (uint32_t)__popcll(mm);
                    }
                }
                bv_lrt_sync<0>();
                const uint32_t w0 = stage[lane], w1 = stage[64 + lane];
                dst[lane] = w0;
                dst[64 + lane] = w1;
                n_stores = 3u;
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
#pragma unroll
                    for (int qr = 0; qr < 2; ++qr) {
                        const unsigned long long mm = m[b * 2 + qr];
                        const uint32_t pos = pos0 + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
                        if (c[b][qr] != 0u) dst[pos] = ((((uint32_t)b << 7) | ((uint32_t)qr << 6)) << 16) | lane16 | c[b][qr];
                        pos0 += (uint32_t)__popcll(mm);
                    }
                }
                n_stores = 0u;  // not counted: the waits that follow are the conservative ones
            }
        }
        {
            // 48-byte summary: 12 lanes, one dword each
            const uint32_t fl = q0_mask | (badq ? BV_SUM_BADQ : 0u) | (is_cand ? BV_SUM_CAND : 0u);
            uint32_t w = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                w = (lane == b) ? fwd[b] : w;
                w = (lane == 4 + b) ? rev[b] : w;
            }
            w = (lane == 8) ? nb : w;
            w = (lane == 9) ? fl : w;
            if (lane < 12) reinterpret_cast<uint32_t *>(&a.summ[site])[lane] = w;
        }
        prev_site = site;
        prev_kind = (uint32_t)__builtin_amdgcn_readfirstlane((int)kind);
        wsel = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_stores);
        } else {
        // ---- a variant site's two rank sums (ref_vs_alt_ranksumtest on mapq and read-position rank, caller.cpp:1151-1154) from
        // the [class][256] histograms, as exact integers; their phred values are formed for up to 64 rows at a time
        wsel = 0u;
        const unsigned long long n12 = (unsigned long long)(c_y & 0xFFFFu) + (unsigned long long)(c_y >> 16);
        if (__ballot(hi_acc != 0u) != 0ull) {
            // a rank >= 256 somewhere in the row (long reads): re-done at once by the exact window sweeps (the ring drains -- rare)
            const BvFusedPlanes pl = bv_f_planes(a, site);
            bv_f_p2_redo(pl.bs, pl.mq, pl.rp, a.out, a.pitch, a.n_samples, site, c_z | (tag ? 0x80000000u : 0u), c_y, (uint32_t)(uintptr_t)(bv_lds_u32 *)hist);
        } else {
            // (these two sums into the stash stand in bv_f_p2_rows too: as one function for both, bv_p1s_fused_kernel<true> -- the
            // caller of both, its registers allotted around theirs -- spilled a register it does not spill now)
            uint32_t *hm = hist, *hr = hist + 512;
            unsigned long long below = 0, twoR = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) twoR += bv_ranksum_window(hm[w * 64 + lane], hm[256 + w * 64 + lane], n12, below, lane);
            stash.tw_m = ((uint32_t)lane == stash.n) ? twoR : stash.tw_m;
            below = 0; twoR = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) twoR += bv_ranksum_window(hr[w * 64 + lane], hr[256 + w * 64 + lane], n12, below, lane);
            stash.tw_r = ((uint32_t)lane == stash.n) ? twoR : stash.tw_r;
            stash.site = ((uint32_t)lane == stash.n) ? site : stash.site;
            stash.n12 = ((uint32_t)lane == stash.n) ? c_y : stash.n12;
            if (++stash.n == 64u) bv_f_stash_flush(a, stash, lane);
        }
        }
        // ---- hand the histogram back, zeroed
        bv_p1s_zero_hist<true>(hist, lane);
        bv_lrt_sync<0>();
        if (is_p1) BV_PH(5); else BV_PH(6);
        if (st & N_HAVE) { c_site = n_site; c_kind = n_kind; c_x = n_x; c_y = n_y; c_z = n_z; st &= ~N_HAVE; }
        else st &= ~C_HAVE;
        // the last pass-1 row of this wave is behind it: publish it, count the wave
        if ((st & CUR_DONE) && !(st & P1_FIN) && !((st & C_HAVE) && c_kind == BV_FK_P1) && !((st & N_HAVE) && n_kind == BV_FK_P1)) finish_p1();
    }
    // ---- no row in flight: the ring is idle
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (prev_kind != 0u) {  // (a pass-1 row whose successor was not drawn yet: the variant queue had priority and was emptied by another wave)
        bv_f_publish(a, sh, B0, prev_site, prev_kind, lane);
        if (prev_kind == 4u) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        prev_kind = 0;
        if (lane == 0 && !(st & (P1_FIN | CUR_DONE))) {
            const uint32_t cur_now = bv_f_lds_read_u(&sh.ctl[BV_FC_CURSOR]);
            sh.pub[wave] = cur_now < B1 - B0 ? B0 + cur_now : 0xFFFFFFF0u;
        }
    }
    if ((st & CUR_DONE) && !(st & P1_FIN)) finish_p1();
    if (P2RING && stash.n != 0u) bv_f_stash_flush(a, stash, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    BV_PH(8);
    BV_PH_FLUSH(a.counters, lane);
    (void)c_z;
    return st & (P_DONE | CUR_DONE | P1_FIN);
}
