// bv_short_stream.h -- the streaming kernel of the two-kernel short-row form: bv_p1s_stream_kernel, its workgroup state and the
// tally of one ring slot.
// Included by bv_pass1_short.hip alone, behind bv_short.h; launched by bv_launch_p1s_stream.
#pragma once

// ------------------------------------------------------------------------------ streaming kernel
#define BV_S_REFCAP 4096                     /* sites of a workgroup's range handled per pass (their reference bases sit in LDS) */
template <int NW, int K, int U>
struct __attribute__((aligned(16))) BvP1sStreamShared {
    uint32_t hist[NW][BV_S_HWORDS + BV_S_OVF + 8];     // per wave: [(rev<<2)|base][phred < 128], then the overflow rows
    uint32_t ring[NW][K][U * BV_S_SLOT_WORDS];         // per wave: K slots of U x (1 KiB calls + 1 KiB phreds)
    uint8_t refl[BV_S_REFCAP];                         // reference bases of the workgroup's current sites
    uint32_t cursor;                                   // sites of the current pass handed out so far
};

// One slot of one row: tally its 64 x 16 cells into the wave's histogram.
template <bool LAST>
__device__ __forceinline__ void bv_p1s_tally_slot(bv_u32x4 vb, bv_u32x4 vq, uint32_t chunk, uint32_t n_chunks, int tail,
                                                  uint32_t *hist, uint32_t one) {
    if (LAST) {
        // the row's last slot: lanes past the row were not loaded (their LDS bytes are stale), and the last chunk may be partial
        if (chunk >= n_chunks) {
            vb = bv_u32x4{0x08080808u, 0x08080808u, 0x08080808u, 0x08080808u};
            vq = bv_u32x4{0u, 0u, 0u, 0u};
        } else if (tail && chunk == n_chunks - 1) {
            vb.x = bv_mask_tail_dword(vb.x, tail);
            vb.y = bv_mask_tail_dword(vb.y, tail - 4);
            vb.z = bv_mask_tail_dword(vb.z, tail - 8);
            vb.w = bv_mask_tail_dword(vb.w, tail - 12);
        }
    }
    // A phred byte >= 128 (invalid input) would carry into its neighbour under the shift below: such a slot takes the
    // exact cell-by-cell path (wave-uniform branch; never taken on valid data).
    const uint32_t hi = (vq.x | vq.y | vq.z | vq.w) & 0x80808080u;
    if (__builtin_expect(__ballot(hi != 0u) != 0ull, 0)) {
        const uint32_t wb[4] = {vb.x, vb.y, vb.z, vb.w}, wq[4] = {vq.x, vq.y, vq.z, vq.w};
#pragma unroll 1
        for (int j = 0; j < 16; ++j) {
            const uint32_t c = (wb[j >> 2] >> (8 * (j & 3))) & 0xFFu, p = (wq[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            if (c < 8u) atomicAdd(p < 128u ? &hist[(c << 7) | p] : &hist[BV_S_HWORDS + c], 1u);
        }
        return;
    }
    // X = call << 8 | phred << 1 = twice the word index of the 8 x 128 histogram; call < 8 <=> X < 0x800
    vq.x <<= 1; vq.y <<= 1; vq.z <<= 1; vq.w <<= 1;
    bv_tally_chunk<1>(vb, vq, hist, one);
}

#define BV_P1S_NW 4
template <int NW, int K, int U, bool CHAIN = false>
__global__ __launch_bounds__(BV_WAVE *NW) void bv_p1s_stream_kernel(BvP1ShortArgs a) {
    __shared__ BvP1sStreamShared<NW, K, U> sh;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *hist = sh.hist[wave];
    const uint32_t ring_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(bv_lds_u32 *)sh.ring[wave][0]);
    const uint32_t *ring = sh.ring[wave][0];
    const uint32_t cursor_lds = (uint32_t)(uintptr_t)(bv_lds_u32 *)&sh.cursor;
    {
        uint4 *h4 = reinterpret_cast<uint4 *>(hist);
#pragma unroll
        for (int i = 0; i < (BV_S_HWORDS + BV_S_OVF + 8) / 4 / BV_WAVE + 1; ++i)
            if (i * BV_WAVE + lane < (BV_S_HWORDS + BV_S_OVF + 8) / 4) h4[i * BV_WAVE + lane] = make_uint4(0, 0, 0, 0);
    }
    // The WORKGROUP owns a contiguous range of sites; its waves draw chunks of C consecutive sites from a cursor in LDS.
    // (Each wave used to own a fixed range of its own.  Measured with per-wave time stamps: of the two waves that share a
    // SIMD the one in wave slot 0 -- the older one, which the issue arbiter prefers -- was done after 303 us, the one in
    // slot 1 after 360 us, and the kernel lasted as long as the slower half.  Drawing the work in small chunks lets the
    // favoured waves take more of it; an LDS atomic per chunk does not touch vmcnt, so the ring keeps its counted waits.)
    const uint32_t B0 = (uint32_t)((uint64_t)a.n_sites * blockIdx.x / gridDim.x), B1 = (uint32_t)((uint64_t)a.n_sites * (blockIdx.x + 1) / gridDim.x);
#ifdef BV_TEAM_DEBUG  /* per-wave end stamps, per-workgroup start stamp and XCD (tools/experiments/r3_team_debug.sh) */
    const uint32_t gw = blockIdx.x * NW + (uint32_t)wave;
    uint32_t *dbg_ = a.counters + BV_CTR_WORDS;
    if (gridDim.x * NW <= 2048u) {
        if (threadIdx.x == 0 && blockIdx.x == 0) dbg_[5150] = 1u;  // whose stamps these are
        if (threadIdx.x == 0) { dbg_[4096 + blockIdx.x] = (uint32_t)__builtin_amdgcn_s_memrealtime(); dbg_[4608 + blockIdx.x] = __builtin_amdgcn_s_getreg((31 << 11) | 20); }
        if (lane == 0) dbg_[2048 + gw] = __builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_ID
    }
#endif
    const uint32_t n_chunks = (a.n_samples + 15u) >> 4, n_slots = (n_chunks + 64u * U - 1u) / (64u * U);
    const int tail = (int)(a.n_samples & 15u);
    const uint32_t voff = (uint32_t)lane * 16u;
    const uint32_t last_valid = n_chunks - (n_slots - 1u) * 64u * U;  // chunks of a row's last slot that lie inside the row
    // a chunk is at least K slots long, so the loads in flight never reach past the chunk after the one being tallied
    uint32_t C = 1u;  // = ceil(K / n_slots), without a division (its VALU expansion would drag the ring's scalar state into VGPRs)
    while (C * n_slots < (uint32_t)K) ++C;
    uint32_t one;
    asm volatile("v_mov_b32 %0, 1" : "=v"(one));

    uint32_t ring_w = 0, ring_r = 0, inflight = 0;
    uint32_t cand = 0, n_cand = 0;  // lane k: the k-th wave-solver candidate of this wave since the last flush
    uint32_t easy = 0, n_easy = 0;  // the same for the candidates of the 16-lane solver (<= 2 active bases)
    uint32_t easy3 = 0, n_easy3 = 0;  //                                                  (>= 3 active bases)
#pragma unroll 1
    for (uint32_t e0 = B0; e0 < B1; e0 += (uint32_t)BV_S_REFCAP) {  // one pass unless the workgroup has more than BV_S_REFCAP sites
    const uint32_t e1 = (B1 - e0 > (uint32_t)BV_S_REFCAP) ? e0 + (uint32_t)BV_S_REFCAP : B1;
    __syncthreads();  // (a later pass: every wave is done with refl and the cursor)
    for (uint32_t i = 0; i < e1 - e0; i += BV_WAVE * NW)  // (uniform trip count: a divergent loop here makes the compiler treat the ring state as per-lane)
        if (i + threadIdx.x < e1 - e0) sh.refl[i + threadIdx.x] = a.ref_base[e0 + i + threadIdx.x];
    if (threadIdx.x == 0) sh.cursor = 0u;
    __syncthreads();

    // prefetch cursor: the next slot to request, inside the chunk [p_site, p_end)
    uint32_t p_site = 0, p_end = 0, p_j = 0;
    // the chunk being tallied and the one after it (drawn by the prefetch side, which runs ahead)
    uint32_t c_site = 0, c_end = 0, n_site = 0, n_end = 0;
    // bit 0: no chunks left to draw; bit 1: [c_site, c_end) is valid; bit 2: [n_site, n_end) is valid.  (One word, not three
    // bools: the optimiser merged the bools' stores into one store through a selected pointer, which kept them -- and with
    // them everything the prefetch step computes -- in scratch memory and VGPRs.)
    uint32_t st = 0;
    constexpr uint32_t P_DONE = 1u, C_HAVE = 2u, N_HAVE = 4u;
    const uint8_t *seg_bs = a.bs, *seg_q = a.q;  // CHAIN: the (biased) planes of the segment that holds p_site
    auto issue = [&]() __attribute__((always_inline)) {  // (out of line its captured state would live in scratch memory)
        if (p_site == p_end) {
            if (st & P_DONE) return;
            const uint32_t c = bv_lds_fetch_add_wave(cursor_lds, C);
            if (c >= e1 - e0) { st |= P_DONE; return; }
            p_site = e0 + c; p_end = (e1 - p_site > C) ? p_site + C : e1; p_j = 0;
            if (!(st & C_HAVE)) { c_site = p_site; c_end = p_end; st |= C_HAVE; }
            else { n_site = p_site; n_end = p_end; st |= N_HAVE; }
        }
        {
            if (CHAIN && p_j == 0u) {
                const BvChainC ch = bv_chain_const(a.ch);
                const uint32_t sg = bv_chain_seg_uniform(ch, p_site);
                seg_bs = ch->bs[sg]; seg_q = ch->q[sg];
            }
            const size_t off = (size_t)p_site * a.pitch + (size_t)p_j * (1024u * U);
            const uint8_t *pb = bv_uniform_ptr(seg_bs + off), *pq = bv_uniform_ptr(seg_q + off);
            const uint32_t dst = ring_lds + ring_w * (U * BV_S_SLOT_WORDS * 4u);
#pragma unroll
            for (int u = 0; u < U; ++u) {  // slot layout: U KiB of calls, then U KiB of phreds
                // Every slot issues exactly 2 U loads (the counted waits rely on it): a KiB that lies wholly past the row's
                // end is "loaded" by lane 0 alone from the row's first bytes (its cells are masked in the tally)
                const bool any = p_j + 1u < n_slots || 64u * u < last_valid;
                const uint8_t *sb = any ? pb + 1024u * u : bv_uniform_ptr(seg_bs + (size_t)p_site * a.pitch);
                const uint8_t *sq = any ? pq + 1024u * u : bv_uniform_ptr(seg_q + (size_t)p_site * a.pitch);
                if (any ? (p_j + 1u < n_slots || (uint32_t)lane + 64u * u < last_valid) : lane == 0) {  // chunks past the row's end load nothing
                    bv_glds16(dst + 1024u * u, sb, voff);
                    bv_glds16(dst + 1024u * (U + u), sq, voff);
                }
            }
            ring_w = (ring_w + 1u == (uint32_t)K) ? 0u : ring_w + 1u;
            ++inflight;
            if (++p_j == n_slots) { p_j = 0; ++p_site; }
        }
    };
#pragma unroll 1
    for (int k = 0; k < K; ++k) issue();

#pragma unroll 1
    while (st & C_HAVE) {
#pragma unroll 1
    for (uint32_t site = c_site; site < c_end; ++site) {
#pragma unroll 1
        for (uint32_t j = 0; j < n_slots; ++j) {
            // the oldest slot in flight has landed once at most 2 (K - 1) younger loads are outstanding
            if (inflight == (uint32_t)K) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * U * (K - 1)) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            bv_u32x4 vb[U], vq[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                vb[u] = *reinterpret_cast<const bv_u32x4 *>(ring + ring_r * (U * BV_S_SLOT_WORDS) + u * 256 + lane * 4);
                vq[u] = *reinterpret_cast<const bv_u32x4 *>(ring + ring_r * (U * BV_S_SLOT_WORDS) + (U + u) * 256 + lane * 4);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // in registers: the slot may be refilled
            ring_r = (ring_r + 1u == (uint32_t)K) ? 0u : ring_r + 1u;
            --inflight;
            issue();
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t chunk = (j * U + u) * 64u + (uint32_t)lane;
                if (j + 1u == n_slots) bv_p1s_tally_slot<true>(vb[u], vq[u], chunk, n_chunks, tail, hist, one);
                else bv_p1s_tally_slot<false>(vb[u], vq[u], chunk, n_chunks, tail, hist, one);
            }
        }
        bv_lrt_sync<0>();

        // ---- the row's totals (LDS operations of one wave execute in order: the adds above are done)
        uint32_t c[4][2], facc[4], racc[4];
        bool bad = false;
        uint32_t q0_mask = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
#pragma unroll
            for (int qr = 0; qr < 2; ++qr) {
                const int q = (qr << 6) | lane;
                const uint32_t f = hist[(b << 7) | q], v = hist[((b | 4) << 7) | q];
                c[b][qr] = f + v;
                if (qr == 0) { facc[b] = f; racc[b] = v; } else { facc[b] += f; racc[b] += v; }
                if (qr == 1) bad |= (c[b][qr] != 0u) && (q >= BV_NQ_VALID);
            }
            if (__builtin_amdgcn_readfirstlane((int)c[b][0]) != 0) q0_mask |= 1u << b;
        }
        uint32_t fwd[4], rev[4];
        {
            const uint32_t v[8] = {facc[0], facc[1], facc[2], facc[3], racc[0], racc[1], racc[2], racc[3]};
            uint32_t t[8];
            bv_wave_sum8_u32(v, t, lane);
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

        // ---- candidate or not.  Not a candidate: nothing covered, or exactly one active base (basetype.cpp:135-139), it is
        // the reference base, none of its calls has phred 0, and the all-sites strand table is shallow.
        bool is_cand = false;
        uint32_t n_active = 0;
        if (total != 0u && !(a.flags & BV_FLAG_TALLY_ONLY)) {
            const int bsel = lane & 3;
            const bool act = (double)bv_sel4u(depth, bsel) / (int)total >= a.min_af;  // basetype.cpp:137, one base per lane
            const uint32_t act_mask = (uint32_t)(__ballot(act) & 0xFull);
            n_active = (uint32_t)__popc(act_mask);
            int ref = __builtin_amdgcn_readfirstlane((int)sh.refl[site - e0]);
            if (ref > 4) ref = 4;
            const bool one_ref = act_mask != 0u && (act_mask & (act_mask - 1u)) == 0u && ref < 4 && act_mask == (1u << ref);
            is_cand = !one_ref || (q0_mask & act_mask) != 0u;
            if (!is_cand) {
                // Fisher tables of (ref_fwd, ref_rev, alt_fwd, alt_rev): imax - imin + 1 (kfunc.c:253-257)
                const uint32_t rf = bv_sel4u(fwd, ref), rr = bv_sel4u(rev, ref);
                const uint32_t af = fwd[0] + fwd[1] + fwd[2] + fwd[3] - rf, ar = rev[0] + rev[1] + rev[2] + rev[3] - rr;
                const int n1_ = (int)(rf + rr), n_1 = (int)(rf + af), n = (int)total;
                const int imax = n_1 < n1_ ? n_1 : n1_;
                int imin = n1_ + n_1 - n;
                if (imin < 0) imin = 0;
                (void)ar;
                is_cand = (imax - imin + 1) > BV_S_SIMPLE_MAX_TABLES;
            }
        }
        uint32_t nb = 0;
        if (is_cand) {
            // every non-empty (base, phred < 128) bin, in (base, phred) order -- the order of bv_prologue_wave
            uint32_t *dst = a.bins + (size_t)site * BV_S_BIN_STRIDE;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
#pragma unroll
                for (int qr = 0; qr < 2; ++qr) {
                    const int q = (qr << 6) | lane;
                    const bool valid = c[b][qr] != 0u;
                    const unsigned long long m = __ballot(valid);
                    const uint32_t pos = nb + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    if (valid) dst[pos] = ((((uint32_t)b << 7) | (uint32_t)q) << 16) | c[b][qr];
                    nb += (uint32_t)__popcll(m);
                }
            }
            // four per wave (bv_solver16.h) unless the site needs what only the wave solver has: the ordered replay of a
            // shallow site, the literal 0/0 arithmetic of phred-0 calls or of min_af <= 0, or more than 128 bins
            const bool is_easy = q0_mask == 0u && total > (uint32_t)BV_ORD_MAX && nb <= (uint32_t)BV_G16_MAX_BINS && a.min_af > 0.0 &&
                                 !(a.flags & BV_FLAG_WAVE_SOLVER);
            if (is_easy && n_active <= 2u) { easy = ((uint32_t)lane == n_easy) ? site : easy; ++n_easy; }
            else if (is_easy) { easy3 = ((uint32_t)lane == n_easy3) ? site : easy3; ++n_easy3; }
            else { cand = ((uint32_t)lane == n_cand) ? site : cand; ++n_cand; }
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
        // ---- hand the histogram back, zeroed
        bv_p1s_zero_hist<true>(hist, lane);
        bv_lrt_sync<0>();
        // a full list of this wave's candidates is flushed: one atomic reserves their places in the list
        if (n_cand == 64u) { bv_p1s_flush_list(&a.counters[BV_CTR_CANDS], a.cand_list, cand, n_cand, lane); n_cand = 0; }
        if (n_easy == 64u) { bv_p1s_flush_list(&a.counters[BV_CTR_EASY], a.easy_list, easy, n_easy, lane); n_easy = 0; }
        if (n_easy3 == 64u) { bv_p1s_flush_list(&a.counters[BV_CTR_EASY3], a.easy3_list, easy3, n_easy3, lane); n_easy3 = 0; }
    }  // sites of the chunk
        if (st & N_HAVE) { c_site = n_site; c_end = n_end; st &= ~N_HAVE; }
        else st &= ~C_HAVE;
    }  // chunks
    }  // passes
    // what is left of this wave's candidate lists (the wait for an atomic's return drains the ring: empty by now)
    if (n_cand != 0u) bv_p1s_flush_list(&a.counters[BV_CTR_CANDS], a.cand_list, cand, n_cand, lane);
    if (n_easy != 0u) bv_p1s_flush_list(&a.counters[BV_CTR_EASY], a.easy_list, easy, n_easy, lane);
    if (n_easy3 != 0u) bv_p1s_flush_list(&a.counters[BV_CTR_EASY3], a.easy3_list, easy3, n_easy3, lane);
#ifdef BV_TEAM_DEBUG
    if (gridDim.x * NW <= 2048u && lane == 0) dbg_[gw] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
}
