// bv_fused_p2rows.h -- the fused short-row kernel's pass-2 rows tallied from registers (bv_f_p2_rows) and what only it uses.
// Included by bv_pass1_fused.hip alone, last of the pieces: behind bv_fused_stream.h (BvFusedStash, bv_f_p2_redo, bv_f_args, bv_f_planes);
// the kernel shell calls bv_f_p2_rows from streaming and solver waves.
#pragma once

// ------------------------------------------------------------------------------ pass-2 rows, tallied from REGISTERS
// Behind the last pass-1 row the launch is ~140 us of the variant sites' rank-sum rows and of the solver's last jobs, and that phase
// is issue-bound: two streaming waves per SIMD tallying (~170 instructions per 1,024 cells and wave) beside a solver wave that runs
// out of jobs 70-100 us in.  Here those rows come by plain non-temporal loads, two blocks of 1,024 cells in flight
// per wave -- no ring, no LDS-DMA: all a wave needs is a 4 KiB histogram -- so the SOLVER waves, out of jobs, tally them too (their
// group scratch is the histogram): half as many waves again on every SIMD for the launch's last stretch.  Same tally, same epilogue,
// same records as the ring's pass-2 slots (bv_f_stream_until_idle).  For the tagged rank layout (BV_SLAB_RPR_TAGGED: mapq + ranks,
// the class of a cell from its rank word); rows of the plain layout, and every row with BV_FLAG_P2_TAIL_DMA (A/B, tests), keep the ring.
// Returns when no variant row can be had right now, or -- candidates first -- when a candidate waits for a solver.
struct BvP2Blk {
    bv_u32x4 w1, w2, w3;  // 16 cells per lane: mapq, ranks 0-7, ranks 8-15 (tagged: no call plane)
};
// 16 bytes of a plane, non-temporal, as a GLOBAL load (a generic pointer makes a flat one, which the compiler can only wait for with
// vmcnt(0) and lgkmcnt(0): no second block in flight under the first one's tally)
__device__ __forceinline__ bv_u32x4 bv_f_ntload16(const uint8_t *base, uint32_t off) {
    typedef const __attribute__((address_space(1))) bv_u32x4 *gp;
    return __builtin_nontemporal_load((gp)(uintptr_t)(base + off));
}
__device__ __attribute__((noinline, not_tail_called)) void bv_f_p2_rows(uint32_t ka_lo_, uint32_t ka_hi_, uint32_t sh_lds_, uint32_t hist_lds_, uint32_t B0_) {
    const uint32_t sh_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh_lds_);
    const uint32_t hist_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)hist_lds_);
    const uint32_t B0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)B0_);
    BvFusedShared &sh = *(BvFusedShared *)(__attribute__((address_space(3))) BvFusedShared *)(uintptr_t)sh_lds;
    uint32_t *hist = (uint32_t *)(__attribute__((address_space(3))) uint32_t *)(uintptr_t)hist_lds;  // [2][256] mapq, [2][256] ranks: zero on entry, zero on return
    const BvP1ShortArgs a = bv_f_args(ka_lo_, ka_hi_);
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t qvhead_lds = (uint32_t)(uintptr_t)(bv_lds_u32 *)&sh.ctl[BV_FC_QV_HEAD];
    const uint32_t ovhead_lds = (uint32_t)(uintptr_t)(bv_lds_u32 *)&sh.ctl[BV_FC_OV_HEAD];
    const uint32_t n_chunks = (a.n_samples + 15u) >> 4;
    const int tail = (int)(a.n_samples & 15u);
    const uint32_t n_blk = (n_chunks + 63u) >> 6;
    const uint32_t last2 = n_chunks - (n_blk - 1u) * 64u;  // chunks of a row's last block: 1 .. 64
    const uint32_t hi_mask = bv_rpr_hi_mask(1u);
    uint32_t one;
    asm volatile("v_mov_b32 %0, 1" : "=v"(one));
    BvFusedStash stash;
    stash.site = 0; stash.n12 = 0; stash.tw_m = 0; stash.tw_r = 0; stash.n = 0;
    // a row: the variant site's facts (class table, REF / ALT depths, the window sweeps' 2-bit table) and its planes
    struct Row {
        uint32_t site, L, n12w, lut;
        const uint8_t *pm, *pr;
        BvFusedPlanes pl;
    };
    // a variant site from the queue in LDS, else from the overflow list (as bv_f_stream_until_idle draws them); false: none right now
    auto pop = [&](Row &r) __attribute__((always_inline)) -> bool {
#pragma unroll 1
        for (;;) {
            const uint32_t h = bv_f_lds_read_u(&sh.ctl[BV_FC_QV_HEAD]);
            if (h != bv_f_lds_read_u(&sh.ctl[BV_FC_QV_TAIL])) {
                if (bv_f_lds_cas_wave(qvhead_lds, h, h + 1u) != h) continue;  // (another wave took it: look again)
                const uint32_t *e = sh.qv[h & (BV_F_QVCAP - 1u)];
                uint32_t site = BV_F_EMPTY;
                for (uint32_t spins = 0; (site = bv_f_lds_read_u(&e[0])) == BV_F_EMPTY && spins < BV_F_SPIN_MAX; ++spins) __builtin_amdgcn_s_sleep(4);
                r.L = bv_f_lds_read_u(&e[1]); r.n12w = bv_f_lds_read_u(&e[2]); r.lut = bv_f_lds_read_u(&e[3]);
                if (lane == 0) *(bv_lds_vu32 *)&e[0] = BV_F_EMPTY;
                if (site == BV_F_EMPTY) { if (lane == 0) atomicOr(&a.counters[BV_CTR_TIMEOUT], BV_TMO_TAKE_VARIANT); continue; }  // (timed out: flagged)
                r.site = site;
            } else {
                const uint32_t oh = bv_f_lds_read_u(&sh.ctl[BV_FC_OV_HEAD]);
                if (oh == bv_f_lds_read_u(&sh.ctl[BV_FC_OV_TAIL])) return false;
                if (bv_f_lds_cas_wave(ovhead_lds, oh, oh + 1u) != oh) continue;
                bv_u32x4 e;  // (through the L2: the entry was written by a solver wave of this workgroup)
                asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(e) : "v"(a.ovf + 4u * (size_t)(B0 + oh)) : "memory");
                r.site = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.x); r.L = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.y);
                r.n12w = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.z); r.lut = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.w);
            }
            r.pl = bv_f_planes(a, r.site);
            const uint64_t off = (uint64_t)r.site * a.pitch;
            r.pm = bv_uniform_ptr(r.pl.mq + off);
            r.pr = bv_uniform_ptr(reinterpret_cast<const uint8_t *>(r.pl.rp) + 2u * off);
            return true;
        }
    };
    // The rows as ONE stream of blocks, a row on an even number of positions (an odd row's last position is read again and not
    // tallied), even positions in A, odd ones in B: position g of the current row -- or, from g = n_even on, position g - n_even of the
    // NEXT row, so that a row's first two blocks are in flight under the epilogue of the row before it.  Every load UNCONDITIONAL (a
    // block past the last row's end is that row's last block again; a lane past the end of a last block reads the block's last
    // valid chunk -- in bounds, and replaced by cells that count nowhere before the tally looks at it): behind a branch the compiler
    // waits for everything in flight, in straight-line code it counts.
    const uint32_t n_even = (n_blk + 1u) & ~1u;
    Row cur, nxt;
    bool have_nxt = false;
    auto load_pos = [&](uint32_t g, BvP2Blk &W) __attribute__((always_inline)) {
        const bool in_next = g >= n_even && have_nxt;
        uint32_t b = in_next ? g - n_even : g;
        b = b < n_blk ? b : n_blk - 1u;
        const uint8_t *pm = in_next ? nxt.pm : cur.pm, *pr = in_next ? nxt.pr : cur.pr;
        const uint32_t ln = (b + 1u == n_blk && (uint32_t)lane >= last2) ? last2 - 1u : (uint32_t)lane;
        W.w1 = bv_f_ntload16(pm + (size_t)b * 1024u, ln * 16u);
        W.w2 = bv_f_ntload16(pr + (size_t)b * 2048u, ln * 32u);
        W.w3 = bv_f_ntload16(pr + (size_t)b * 2048u, ln * 32u + 16u);
    };
    BvP2Blk A, B;
    bool have = pop(cur);
    if (have) {
        load_pos(0u, A);
        load_pos(1u, B);
    }
#pragma unroll 1
    while (have) {
        const uint32_t site = cur.site, L = cur.L, n12w = cur.n12w;
        const bool deep = ((n12w & 0xFFFFu) + (n12w >> 16)) * 8u >= a.n_samples && !(a.flags & BV_FLAG_NO_DOM);
        uint32_t hi_acc = 0, dom = BV_DOM_NONE;
        // the tally of a block, as the ring's pass-2 slots are tallied (bv_f_stream_until_idle)
        auto tally_blk = [&](uint32_t b, BvP2Blk &W) __attribute__((always_inline)) {
            const bool lastb = b + 1u == n_blk;
            if (lastb) {
                if ((uint32_t)lane >= last2) W.w1 = bv_u32x4{0u, 0u, 0u, 0u};  // (not the lane's own cells: see load_pos)
                bv_f_p2t_last(W.w2, W.w3, lane, last2, tail);
            }
            uint32_t c0, c1, c2, c3;
            bv_p2t_class16(L, W.w2, W.w3, c0, c1, c2, c3);
            // ranks that do not fit the 256-rank window: remembered, the row is then re-done by the window sweeps
            hi_acc |= (W.w2.x | W.w2.y | W.w2.z | W.w2.w | W.w3.x | W.w3.y | W.w3.z | W.w3.w) & hi_mask;
            uint32_t x[16], y[16];
            bv_p2d_xy16(c0, c1, c2, c3, W.w1, W.w2, W.w3, x, y);
            bv_p2d_add16(x, y, hist, hist + 512, one, deep, dom);
        };
#pragma unroll 1
        for (uint32_t b = 0; b < n_even; b += 2u) {
            tally_blk(b, A);
            if (b + 2u == n_even) {
                // the row's last pair: the next row is drawn here, its first two blocks are requested below -- unless a candidate waits:
                // the solver's jobs come first (see the kernel's loop), and the wave leaves behind this row's epilogue
                const bool cand = bv_f_lds_read_u(&sh.ctl[BV_FC_Q3_TAIL]) != bv_f_lds_read_u(&sh.ctl[BV_FC_Q3_HEAD]) ||
                                  bv_f_lds_read_u(&sh.ctl[BV_FC_Q2_TAIL]) != bv_f_lds_read_u(&sh.ctl[BV_FC_Q2_HEAD]);
                have_nxt = !cand && pop(nxt);
            }
            load_pos(b + 2u, A);
            if (b + 1u < n_blk) tally_blk(b + 1u, B);
            load_pos(b + 3u, B);
        }
        bv_lrt_sync<0>();
        // ---- the site's two rank sums (as in bv_f_stream_until_idle)
        const unsigned long long n12 = (unsigned long long)(n12w & 0xFFFFu) + (unsigned long long)(n12w >> 16);
        if (__ballot(hi_acc != 0u) != 0ull) {
            bv_f_p2_redo(cur.pl.bs, cur.pl.mq, cur.pl.rp, a.out, a.pitch, a.n_samples, site, cur.lut | 0x80000000u, n12w, hist_lds);
        } else {
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
            stash.n12 = ((uint32_t)lane == stash.n) ? n12w : stash.n12;
            if (++stash.n == 64u) bv_f_stash_flush(a, stash, lane);
        }
        bv_p1s_zero_hist<false>(hist, lane);
        bv_lrt_sync<0>();
        have = have_nxt;
        cur = nxt;
        have_nxt = false;
    }
    if (stash.n != 0u) bv_f_stash_flush(a, stash, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
