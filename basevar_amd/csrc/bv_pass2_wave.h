// bv_pass2_wave.h -- the wave-per-row family of pass 2 (rank sums, no pop-groups): bv_pass2_short_kernel, plain loads, and
// bv_pass2_dma_kernel<TAG>, rows streamed through an LDS ring, with their shared structs and BV_P2S_* / BV_P2D_*.
// Included by bv_pass2.hip alone, behind bv_tally.h and bv_pass2_sweep.h; the launch code there sizes their grids.
#pragma once

// ------------------------------------------------------------------------------ short rows, no pop-groups
// One workgroup launch per variant site costs more than the site itself when a row is a few tens of KB
// (10 k samples: 40 KB).  Here the grid is persistent: four independent waves per workgroup, each with its
// own 4 KiB of histograms (mapq 2 x 256, read-position ranks 2 x 256 per sweep), walk the variant list
// with a fixed stride.  Same arithmetic as bv_pass2_kernel<64, true, false>.
#define BV_P2S_WAVES 4
#define BV_P2S_RW 256
struct __attribute__((aligned(16))) BvPass2ShortShared {
    uint32_t h[BV_P2S_WAVES][2 * 256 + 2 * BV_P2S_RW];  // per wave: hm[2][256] then hr[2][BV_P2S_RW]
};
// The planes the window sweeps read for `site` (they index them with the site number themselves): in a chained launch those of the
// segment that holds the site, biased.  (Short rows: ref_base / out are contiguous either way.)
__device__ __forceinline__ BvPass2Args bv_p2_site_planes(const BvPass2Args &a, uint32_t site) {
    BvPass2Args as = a;
    if (a.ch != nullptr) {
        const BvChainC ch = bv_chain_const(a.ch);
        const uint32_t sg = bv_chain_seg_uniform(ch, site);
        as.bs = ch->bs[sg]; as.mapq = ch->mapq[sg]; as.rpr = ch->rpr[sg];
    }
    return as;
}
__global__ __launch_bounds__(BV_WAVE *BV_P2S_WAVES, 4) void bv_pass2_short_kernel(BvPass2Args a) {
    __shared__ BvPass2ShortShared sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *hm = sh.h[wave], *hr = sh.h[wave] + 2 * 256;
    const uint32_t n_var = a.counters[BV_CTR_VARIANTS];
    const uint32_t stride = gridDim.x * BV_P2S_WAVES;
    for (uint32_t v = blockIdx.x * BV_P2S_WAVES + wave; v < n_var; v += stride) {
        const uint32_t site = a.var_list[v];
        const bv_site_result *res = &a.out[site];
        int ref = a.ref_base[site];
        if (ref > 4) ref = 4;
        const uint32_t depth[4] = {res->depth[0], res->depth[1], res->depth[2], res->depth[3]};
        const uint2 aw = *reinterpret_cast<const uint2 *>(&res->n_alt);
        uint32_t L, lut, n1, n2;
        bv_p2_site_facts(ref, depth, aw.x, aw.y, L, lut, n1, n2);
        bv_p2_wave_exact<BV_P2S_RW>(bv_p2_site_planes(a, site), a.out, site, lut, bv_rpr_rank_mask(a.rpr_tag), n1, n2, hm, hr, lane);
        bv_lrt_sync<0>();
    }
}

// ------------------------------------------------------------------------------ short rows, streamed through LDS
// The same work as bv_pass2_short_kernel for rows of 2,049 .. 49,152 samples, built like the short-row pass 1
// (bv_pass1_short.hip): every wave walks its share of the variant list as ONE sequence of slots -- 1 KiB of calls, 1 KiB of
// mapq, 2 KiB of read-position ranks -- through a private ring in LDS filled by LDS-DMA (no VGPR staging, counted waits, the
// next row already arriving while a row's rank sums are formed), and the per-cell work is cut to the perm form of the tally
// (bv_p2d_xm / bv_p2d_xr, bv_tally.h: the derivation stands there).  A row that holds a rank >= 256 anywhere (long reads; one OR
// per slot finds it) is re-done as bv_pass2_short_kernel does every row (bv_p2_wave_exact).  The site indices and the per-site
// facts pass 1 left (bv_p2_site_facts, formed by each lane for its own site) are fetched for 64 sites at a time, so the ring is
// drained once per 64 sites, not per site.
#define BV_P2D_WAVES 4
#define BV_P2D_K 3
#define BV_P2D_SLOT_WORDS 1024  /* 1 KiB calls, 1 KiB mapq, 2 KiB ranks */
struct __attribute__((aligned(16))) BvPass2DmaShared {
    uint32_t h[BV_P2D_WAVES][4 * 256];                         // per wave: hm[2][256] then hr[2][256]
    uint32_t ring[BV_P2D_WAVES][BV_P2D_K][BV_P2D_SLOT_WORDS];
};

// TAG (BV_SLAB_RPR_TAGGED): a slot is three pieces -- 1 KiB of mapq, 2 KiB of ranks --, the class of a cell comes from the tag in
// its rank word (bv_p2t_class4) and the call plane is not read.
template <bool TAG>
__global__ __launch_bounds__(BV_WAVE *BV_P2D_WAVES) void bv_pass2_dma_kernel(BvPass2Args a) {
    constexpr int PIECES = TAG ? 3 : 4;  // LDS-DMA loads per slot: what the counted waits count
    __shared__ BvPass2DmaShared sh;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *h = sh.h[wave];
    const uint32_t *ring = sh.ring[wave][0];
    const uint32_t ring_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(bv_lds_u32 *)sh.ring[wave][0]);
    const uint32_t n_var = a.counters[BV_CTR_VARIANTS];
    const uint32_t n_waves = gridDim.x * BV_P2D_WAVES, gw = blockIdx.x * BV_P2D_WAVES + (uint32_t)wave;
    if (gw >= n_var) return;
    const uint32_t mine = (n_var - gw + n_waves - 1u) / n_waves;  // variant sites of this wave: gw, gw + n_waves, ...
    const uint32_t n_chunks = (a.n_samples + 15u) >> 4, n_slots = (n_chunks + 63u) >> 6;
    const int tail = (int)(a.n_samples & 15u);
    const uint32_t last_valid = n_chunks - (n_slots - 1u) * 64u;
    const uint32_t voff = (uint32_t)lane * 16u;
    uint32_t one;
    asm volatile("v_mov_b32 %0, 1" : "=v"(one));

    // facts of 64 sites at a time (lane i: the wave's site number blk0 + i)
    uint32_t siteA = 0, siteB = 0;  // site indices of the current and of the next block of 64
    uint32_t fL = 0xFFFFFFFFu, flut = 0xAAu, fn1 = 0, fn2 = 0;  // bv_p2_site_facts of this lane's site of the current block
    auto load_sites = [&](uint32_t blk) -> uint32_t {
        const uint32_t k = blk * 64u + (uint32_t)lane;
        return k < mine ? a.var_list[gw + k * n_waves] : 0u;
    };
    auto site_of = [&](uint32_t k, uint32_t blk0) -> uint32_t {  // k in [blk0, blk0 + 128)
        const uint32_t i = k - blk0;
        return (uint32_t)(i < 64u ? __builtin_amdgcn_readlane((int)siteA, (int)i) : __builtin_amdgcn_readlane((int)siteB, (int)(i - 64u)));
    };
    // prefetch cursor
    uint32_t p_k = 0, p_j = 0, ring_w = 0, inflight = 0, blk0 = 0;
    // a chained launch (a.ch): the planes of the segment that holds the prefetch cursor's site (biased: indexed with the
    // global site number); ref_base / out are contiguous either way
    const uint8_t *seg_bs = a.bs, *seg_mq = a.mapq, *seg_rp = reinterpret_cast<const uint8_t *>(a.rpr);
    auto issue = [&]() {
        if (p_k < mine) {
            const uint32_t site = site_of(p_k, blk0);
            if (a.ch != nullptr && p_j == 0u) {
                const BvChainC ch = bv_chain_const(a.ch);
                const uint32_t sg = bv_chain_seg(ch, site);
                seg_bs = ch->bs[sg]; seg_mq = ch->mapq[sg]; seg_rp = reinterpret_cast<const uint8_t *>(ch->rpr[sg]);
            }
            const size_t row = (size_t)site * a.pitch + (size_t)p_j * 1024u;
            const uint8_t *pb = bv_uniform_ptr(seg_bs + row), *pm = bv_uniform_ptr(seg_mq + row);
            const uint8_t *pr = bv_uniform_ptr(seg_rp + 2u * row);
            const uint32_t dst = ring_lds + ring_w * (BV_P2D_SLOT_WORDS * 4u);
            if (p_j + 1u < n_slots || (uint32_t)lane < last_valid) {  // lanes past the row's end load nothing (lane 0 always loads)
                if (!TAG) bv_glds16(dst, pb, voff);
                bv_glds16(dst + 1024u, pm, voff);
                bv_glds16(dst + 2048u, pr, voff * 2u);         // 32 bytes of ranks per lane: two 16-byte halves
                bv_glds16(dst + 3072u, pr + 16, voff * 2u);
            }
            ring_w = (ring_w + 1u == (uint32_t)BV_P2D_K) ? 0u : ring_w + 1u;
            ++inflight;
            if (++p_j == n_slots) { p_j = 0; ++p_k; }
        }
    };
    siteA = load_sites(0);
    siteB = load_sites(1);
    asm volatile("" : "+v"(siteA), "+v"(siteB)::"memory");
    uint32_t ring_r = 0;
    unsigned long long tw_m = 0, tw_r = 0, fast_mask = 0;  // lane i: twice the REF rank sums of the block's i-th site; bit i: pending
#pragma unroll 1
    for (uint32_t k = 0; k < mine; ++k) {
        if (k == blk0 + 64u) {  // next block of 64 sites (the prefetch cursor is at most one site ahead: n_slots >= K)
            blk0 += 64u;
            siteA = siteB;
            siteB = load_sites(blk0 / 64u + 1u);
            asm volatile("" : "+v"(siteA), "+v"(siteB)::"memory");
        }
        if (k == blk0) {
            // what pass 1 decided for these 64 sites (one drain of the ring per 64 sites)
            const uint32_t kk = k + (uint32_t)lane;
            const uint32_t s_ = kk < mine ? siteA : 0xFFFFFFFFu;
            if (s_ != 0xFFFFFFFFu) {
                const uint4 dd = *reinterpret_cast<const uint4 *>(&a.out[s_].depth[0]);
                const uint2 aw = *reinterpret_cast<const uint2 *>(&a.out[s_].n_alt);
                const uint32_t depth[4] = {dd.x, dd.y, dd.z, dd.w};
                int ref = a.ref_base[s_];
                if (ref > 4) ref = 4;
                bv_p2_site_facts(ref, depth, aw.x, aw.y, fL, flut, fn1, fn2);
            }
            asm volatile("" : "+v"(fL), "+v"(flut), "+v"(fn1), "+v"(fn2)::"memory");
            if (k == 0) {
#pragma unroll 1
                for (int t = 0; t < BV_P2D_K; ++t) issue();
            }
        }
        const int li = (int)(k - blk0);
        const uint32_t site = (uint32_t)__builtin_amdgcn_readlane((int)siteA, li);
        // class table: byte b = class of base b (0x80 REF, 0x81 ALT, 0xFF neither) and the plain 2-bit lut of the sweep code
        const uint32_t L = (uint32_t)__builtin_amdgcn_readlane((int)fL, li), lut = (uint32_t)__builtin_amdgcn_readlane((int)flut, li);
        const unsigned long long n1 = (uint32_t)__builtin_amdgcn_readlane((int)fn1, li), n2 = (uint32_t)__builtin_amdgcn_readlane((int)fn2, li);
        bv_wave_zero<4 * 256>(h, lane);
        uint32_t hi_acc = 0, dom = BV_DOM_NONE;
        const bool deep = (n1 + n2) * 8ull >= (unsigned long long)a.n_samples && !(a.flags & BV_FLAG_NO_DOM);
#pragma unroll 1
        for (uint32_t j = 0; j < n_slots; ++j) {
            if (inflight == (uint32_t)BV_P2D_K) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES * (BV_P2D_K - 1)) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t *sl = ring + ring_r * BV_P2D_SLOT_WORDS;
            bv_u32x4 vb = bv_u32x4{0u, 0u, 0u, 0u};
            if (!TAG) vb = *reinterpret_cast<const bv_u32x4 *>(sl + lane * 4);
            const bv_u32x4 vm = *reinterpret_cast<const bv_u32x4 *>(sl + 256 + lane * 4);
            bv_u32x4 r0 = *reinterpret_cast<const bv_u32x4 *>(sl + 512 + lane * 4);   // ranks 0-7
            bv_u32x4 r1 = *reinterpret_cast<const bv_u32x4 *>(sl + 768 + lane * 4);   // ranks 8-15
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            ring_r = (ring_r + 1u == (uint32_t)BV_P2D_K) ? 0u : ring_r + 1u;
            --inflight;
            issue();
            if (j + 1u == n_slots) {
                const uint32_t chunk = j * 64u + (uint32_t)lane;
                if (chunk >= n_chunks) {  // not loaded: stale bytes
                    vb = bv_u32x4{0x08080808u, 0x08080808u, 0x08080808u, 0x08080808u};
                    r0 = TAG ? bv_u32x4{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u} : bv_u32x4{0u, 0u, 0u, 0u};
                    r1 = r0;
                } else if (tail && chunk == n_chunks - 1) {
                    if (TAG) {
                        bv_p2t_mask_tail16(r0, r1, tail);
                    } else {
                        bv_mask_tail16(vb, tail);
                    }
                }
            }
            // class bytes of the 16 cells (REF 0x00, ALT 0x01, neither >= 0x7F)
            uint32_t c0, c1, c2, c3;
            if (TAG) {
                bv_p2t_class16(L, r0, r1, c0, c1, c2, c3);
            } else {
                c0 = __builtin_amdgcn_perm(L, L, vb.x) ^ 0x80808080u; c1 = __builtin_amdgcn_perm(L, L, vb.y) ^ 0x80808080u;
                c2 = __builtin_amdgcn_perm(L, L, vb.z) ^ 0x80808080u; c3 = __builtin_amdgcn_perm(L, L, vb.w) ^ 0x80808080u;
            }
            // ranks that do not fit the 256-rank window: remembered, the row is then re-done by sweeps (valid data has rank 0
            // in uncovered cells)
            hi_acc |= (r0.x | r0.y | r0.z | r0.w | r1.x | r1.y | r1.z | r1.w) & (TAG ? 0x1F001F00u : 0xFF00FF00u);
            uint32_t x[16], y[16];
            bv_p2d_xy16(c0, c1, c2, c3, vm, r0, r1, x, y);
            bv_p2d_add16(x, y, h, h + 512, one, deep, dom);  // (a deep row: the dominant mapq's lanes are counted, not added one by one)
        }
        bv_lrt_sync<0>();
        uint32_t *hm = h, *hr = h + 512;
        if (__ballot(hi_acc != 0u) != 0ull) {
            // a rank >= 256 somewhere in the row: the exact window sweeps (plain loads; rare -- long reads)
            bv_p2_wave_exact<256>(bv_p2_site_planes(a, site), a.out, site, lut, bv_rpr_rank_mask(a.rpr_tag), n1, n2, hm, hr, lane);
        } else {
            // the two rank sums as exact integers; their phred values (erfc, log10: scalar work) are formed for 64 sites at a
            // time, one site per lane, when the block of sites ends
            unsigned long long below = 0, twoR = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) twoR += bv_ranksum_window(hm[w * 64 + lane], hm[256 + w * 64 + lane], n1 + n2, below, lane);
            tw_m = (lane == li) ? twoR : tw_m;
            below = 0; twoR = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) twoR += bv_ranksum_window(hr[w * 64 + lane], hr[256 + w * 64 + lane], n1 + n2, below, lane);
            tw_r = (lane == li) ? twoR : tw_r;
            fast_mask |= 1ull << li;
        }
        if (li == 63 || k + 1u == mine) {
            if ((fast_mask >> lane) & 1ull) {
                const unsigned long long m1 = fn1, m2 = fn2;  // this lane's site: its own facts
                const double ph_m = bv_ranksum_phred(tw_m, m1, m2), ph_r = bv_ranksum_phred(tw_r, m1, m2);
                a.out[siteA].mq_ranksum = ph_m;
                a.out[siteA].rpr_ranksum = ph_r;
                atomicOr(&a.out[siteA].status, BV_SITE_RANKSUM);
            }
            fast_mask = 0ull;
        }
        bv_lrt_sync<0>();
    }
}
