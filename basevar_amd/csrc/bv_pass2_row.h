// bv_pass2_row.h -- the workgroup-per-row family of pass 2: the workgroup's LDS (BvPass2Shared), the perm-form sweep of a row by the
// whole workgroup (bv_p2_fast_sweep), the steps of bv_pass2_kernel (clear, tally, rank sums, the export of a group as an item, the
// item headers of a site) and the kernel itself, one workgroup per variant site, with or without rank sums and pop-groups.
// Included by bv_pass2.hip alone, behind bv_tally.h and bv_pass2_sweep.h; the launch code there picks the instantiation.
#pragma once

// INLINE: the kernel solves pop-groups itself (one wave per group) and needs the solver's LDS; otherwise every group leaves
// as an item for the group solve kernels and that LDS (and the solver's registers) are not taken.
// RANKS: the kernel forms the rank sums; without them (the group tallies behind a fused pass-1 kernel that has streamed the
// rank-sum rows itself) their 10 KiB are not taken either -- at 32 groups that is a fourth workgroup per CU.
template <int NW, bool INLINE = true, bool RANKS = true>
struct __attribute__((aligned(16))) BvPass2Shared {
    uint32_t hm[RANKS ? 2 * 256 : 4];         // [class][mapq]        class 0 = REF reads, 1 = ALT reads
    uint32_t hr[RANKS ? 2 * BV_RPR_WIN : 4];  // [class][rank - win_lo]
    uint32_t maxr[NW];
    uint32_t bin_code[INLINE ? NW : 1][INLINE ? BV_SLOTS * BV_WAVE : 4];
    uint32_t bin_cnt[INLINE ? NW : 1][INLINE ? BV_SLOTS * BV_WAVE : 4];
    BvLrtShared lrt[INLINE ? NW : 1];
    double tab_hit[INLINE ? BV_QBINS : 2], tab_miss[INLINE ? BV_QBINS : 2];
    alignas(8) uint16_t ord[INLINE ? NW : 1][BV_ORD_ALLOC];  // shallow pop-groups: the group's covered cells in sample order (bv_gather_ordered)
    uint32_t ghdr[INLINE ? 1 : BV_GROUPS_PER_ROUND];  // !INLINE: the header words of the site's items, until the site's kind of small-group solver is known
};

extern __shared__ __attribute__((aligned(16))) uint32_t bv_dyn_lds[];  // hg[n_groups][4][128]

// (BvP2Ctx, bv_p2_dword, bv_p2_sweep -- the window sweeps over a row: bv_pass2_sweep.h)

// (bv_p2d_xm / bv_p2d_xr, the perm form of the rank-sum tally: bv_tally.h)

// One sweep over the row in that form, by the whole workgroup into its shared mapq / rank histograms ([2][256] each; `hr` uses the
// first 512 words of the 1024-rank window) and, with GROUPS, into the per-group (base, phred) histograms `hg`.  Returns this
// thread's OR of what does not fit the form: non-zero somewhere in the workgroup = a rank >= 256 (or a call byte > 15 / a
// phred byte > 127) in the row, the caller re-does the row with the branchy window sweeps (bv_p2_sweep).  L: class table
// (byte b = 0x80 REF / 0x81 ALT / 0xFF neither).  ~6 VALU + 2 predicated ds_add per cell for the rank sums, ~4 + 1 for the
// groups; the branchy sweep takes ~18 VALU for the rank sums alone.
// TAG (rank sums without pop-groups, BV_SLAB_RPR_TAGGED): the class of a cell comes from the tag in its rank word
// (bv_p2t_class4) and the call plane is not read at all -- 3 bytes per cell, SURVEY 8d's figure, instead of 4.
// DOM: the mapq tally takes a dominant value out of the LDS adds (bv_lds_add16_dom): chosen per row by its depth.
template <int NT, bool RANKS, bool GROUPS, bool HALF = false, bool TAG = false, bool DOM = false>
__device__ __forceinline__ uint32_t bv_p2_fast_sweep(const BvPass2Args &a, uint32_t site, int tid, uint32_t L, uint32_t *hm, uint32_t *hr, uint32_t *hg,
                                                     uint32_t *q64 = nullptr /* with GROUPS: this thread's OR of bit 6 of the row's phred bytes */) {
    const size_t row = (size_t)site * a.pitch;
    const bv_u32x4 *b4 = reinterpret_cast<const bv_u32x4 *>(a.bs + row);
    const bv_u32x4 *m4 = RANKS ? reinterpret_cast<const bv_u32x4 *>(a.mapq + row) : nullptr;
    const bv_u32x4 *r4 = RANKS ? reinterpret_cast<const bv_u32x4 *>(a.rpr + row) : nullptr;
    const bv_u32x4 *q4 = GROUPS ? reinterpret_cast<const bv_u32x4 *>(a.q + row) : nullptr;
    const bv_u32x4 *g4 = GROUPS ? reinterpret_cast<const bv_u32x4 *>(a.gidp) : nullptr;  // g << 2, or 0x80: no group
    const uint32_t n_chunks = (a.n_samples + 15u) >> 4;
    const int tail = (int)(a.n_samples & 15u);
    const bv_u32x4 zero = bv_u32x4{0u, 0u, 0u, 0u}, none = bv_u32x4{0x08080808u, 0x08080808u, 0x08080808u, 0x08080808u};
    uint32_t one;
    asm volatile("v_mov_b32 %0, 1" : "=v"(one));
    static_assert(!TAG || (RANKS && !GROUPS), "the tagged form: rank sums without pop-groups");
    const bv_u32x4 nocall = bv_u32x4{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
    const uint32_t hi_mask = TAG ? 0x1F001F00u : bv_rpr_hi_mask(a.rpr_tag);
    uint32_t hi_acc = 0, dom = BV_DOM_NONE, q64_acc = 0;
    // chunks per thread and trip: without the rank planes three loads per chunk, so four chunks -- a 10,000-sample row is then
    // ONE round of loads for a workgroup of 256 (the kernel waits for memory, not for instructions)
    constexpr int U = RANKS ? 2 : 4;
    for (uint32_t base = 0; base < n_chunks; base += NT * U) {
        bv_u32x4 vb[U], vm[U], vr0[U], vr1[U], vq[U], vg[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t idx = base + u * NT + tid;
            vb[u] = none; vm[u] = vr0[u] = vr1[u] = vq[u] = vg[u] = zero;
            if (TAG) vr0[u] = vr1[u] = nocall;
            if (idx < n_chunks) {
                if (!TAG) vb[u] = __builtin_nontemporal_load(b4 + idx);
                if (RANKS) {
                    vm[u] = __builtin_nontemporal_load(m4 + idx);
                    vr0[u] = __builtin_nontemporal_load(r4 + 2 * (size_t)idx);
                    vr1[u] = __builtin_nontemporal_load(r4 + 2 * (size_t)idx + 1);
                }
                if (GROUPS) {
                    vq[u] = __builtin_nontemporal_load(q4 + idx);
                    vg[u] = g4[idx];  // shared by every row: cacheable
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t idx = base + u * NT + tid;
            if (tail && idx == n_chunks - 1) {
                if (TAG) {
                    bv_p2t_mask_tail16(vr0[u], vr1[u], tail);
                } else {
                    bv_mask_tail16(vb[u], tail);
                }
            }
            uint32_t x[16];
            if (RANKS) {
                const bv_u32x4 r0 = vr0[u], r1 = vr1[u], vmq = vm[u];
                uint32_t c0, c1, c2, c3;
                if (TAG) {
                    bv_p2t_class16(L, r0, r1, c0, c1, c2, c3);
                } else {
                    c0 = __builtin_amdgcn_perm(L, L, vb[u].x) ^ 0x80808080u; c1 = __builtin_amdgcn_perm(L, L, vb[u].y) ^ 0x80808080u;
                    c2 = __builtin_amdgcn_perm(L, L, vb[u].z) ^ 0x80808080u; c3 = __builtin_amdgcn_perm(L, L, vb[u].w) ^ 0x80808080u;
                }
                hi_acc |= (r0.x | r0.y | r0.z | r0.w | r1.x | r1.y | r1.z | r1.w) & hi_mask;
                uint32_t y[16];
                bv_p2d_xy16(c0, c1, c2, c3, vmq, r0, r1, x, y);
                // (both histograms under one predicate -- the class byte is the same in x and y -- unless the row is deep and its mapq
                // tally counts the dominant value)
                bv_p2d_add16(x, y, hm, hr, one, DOM, dom);
            }
            if (GROUPS) {
                // the group tally of bv_p2g_stream_kernel: byte = group << 2 | base, bit 7 for "no call" / "no group"; X = byte << 8 |
                // phred << 1 is twice the word index of hg[group][base][128].  Call bytes above 15 and phred bytes above 127 do not
                // fit the packed index: reported like a long read, the row is then re-done by the branchy sweep
                bv_u32x4 q2 = vq[u];
                hi_acc |= ((vb[u].x | vb[u].y | vb[u].z | vb[u].w) & 0xF0F0F0F0u) | ((q2.x | q2.y | q2.z | q2.w) & 0x80808080u);
                q64_acc |= (q2.x | q2.y | q2.z | q2.w) & 0x40404040u;
                const uint32_t y0 = (((vb[u].x & 0x08080808u) << 4) | (vb[u].x & 0x03030303u)) | vg[u].x, y1 = (((vb[u].y & 0x08080808u) << 4) | (vb[u].y & 0x03030303u)) | vg[u].y;
                const uint32_t y2 = (((vb[u].z & 0x08080808u) << 4) | (vb[u].z & 0x03030303u)) | vg[u].z, y3 = (((vb[u].w & 0x08080808u) << 4) | (vb[u].w & 0x03030303u)) | vg[u].w;
                q2.x = (q2.x & 0x7F7F7F7Fu) << 1; q2.y = (q2.y & 0x7F7F7F7Fu) << 1; q2.z = (q2.z & 0x7F7F7F7Fu) << 1; q2.w = (q2.w & 0x7F7F7F7Fu) << 1;
                x[0] = bv_cell_index<0>(y0, q2.x); x[1] = bv_cell_index<1>(y0, q2.x); x[2] = bv_cell_index<2>(y0, q2.x); x[3] = bv_cell_index<3>(y0, q2.x);
                x[4] = bv_cell_index<0>(y1, q2.y); x[5] = bv_cell_index<1>(y1, q2.y); x[6] = bv_cell_index<2>(y1, q2.y); x[7] = bv_cell_index<3>(y1, q2.y);
                x[8] = bv_cell_index<0>(y2, q2.z); x[9] = bv_cell_index<1>(y2, q2.z); x[10] = bv_cell_index<2>(y2, q2.z); x[11] = bv_cell_index<3>(y2, q2.z);
                x[12] = bv_cell_index<0>(y3, q2.w); x[13] = bv_cell_index<1>(y3, q2.w); x[14] = bv_cell_index<2>(y3, q2.w); x[15] = bv_cell_index<3>(y3, q2.w);
                if (HALF) bv_lds_add16_half(x, hg, one, 0x8000u);  // X is the byte offset of a 16-bit counter of hg[group][base][128]
                else bv_lds_add16<1>(x, hg, one, 0x8000u);
            }
        }
    }
    if (GROUPS && q64 != nullptr) *q64 = q64_acc;
    return hi_acc;
}

// ------------------------------------------------------------------------------ the steps of bv_pass2_kernel, in its order
// (SH: the kernel's BvPass2Shared; GW: words of one group's histogram)

// clear: the rank-sum histograms (hm and hr are adjacent and 16-byte aligned) and the n_groups group histograms (GW is a multiple of
// 4 and the dynamic block is 16-byte aligned), with 128-bit stores.  The caller synchronises.
template <int NT, bool RANKS, bool GROUPS, uint32_t GW>
__device__ __forceinline__ void bv_p2_row_clear(uint32_t *hm, uint32_t *hg, uint32_t n_groups, int tid) {
    if (RANKS) {
        uint4 *z = reinterpret_cast<uint4 *>(hm);
        for (int i = tid; i < (2 * 256 + 2 * BV_RPR_WIN) / 4; i += NT) z[i] = make_uint4(0, 0, 0, 0);
    }
    if (GROUPS) {
        uint4 *z = reinterpret_cast<uint4 *>(hg);
        for (uint32_t i = tid; i < n_groups * (GW / 4u); i += NT) z[i] = make_uint4(0, 0, 0, 0);
    }
}

// tally: the perm form first where it applies (rank sums without pop-groups, or groups with the prepared id plane `gidp`: a third
// of the instructions; 256-rank window); a row it does not fit (a rank >= 256: long reads) is cleared and re-done by the window
// sweeps, whose largest classified rank each wave leaves in sh.maxr.  Returns whether the perm form stands.  depth12: the site's
// REF + ALT depth.  lo_only: see below.
template <int NT, bool RANKS, bool GROUPS, bool HALF, bool TAG, class SH>
__device__ __forceinline__ bool bv_p2_row_tally(const BvPass2Args &a, SH &sh, BvP2Ctx &cx, uint32_t site, uint32_t Ltab, uint32_t depth12, int tid,
                                                bool &lo_only) {
    constexpr int NW = NT / BV_WAVE;
    const int lane = tid & 63, wave = tid >> 6;
    const bool FAST = !GROUPS || a.gidp != nullptr;
    bool fast_ok = false;
    lo_only = false;
    if (FAST) {
        // a deep row (an eighth of its cells are REF / ALT reads): most lanes of a wave add to the dominant mapq's word
        const bool deep = RANKS && !GROUPS && (unsigned long long)depth12 * 8ull >= (unsigned long long)a.n_samples && !(a.flags & BV_FLAG_NO_DOM);
        uint32_t q64 = 0;
        const uint32_t hi = deep ? bv_p2_fast_sweep<NT, RANKS, GROUPS, HALF, TAG, RANKS && !GROUPS>(a, site, tid, Ltab, sh.hm, sh.hr, cx.hg)
                                 : bv_p2_fast_sweep<NT, RANKS, GROUPS, HALF, TAG, false>(a, site, tid, Ltab, sh.hm, sh.hr, cx.hg, &q64);
        const bool any_hi = __ballot(hi != 0u) != 0ull, any_q64 = GROUPS && __ballot(q64 != 0u) != 0ull;
        if (lane == 0) sh.maxr[wave] = (any_hi ? 1u : 0u) | (any_q64 ? 2u : 0u);
        __syncthreads();
        uint32_t slow = 0;
        for (int w = 0; w < NW; ++w) slow |= sh.maxr[w];
        fast_ok = (slow & 1u) == 0u;
        // no phred byte of the row has bit 6 or 7 set (every Illumina row: phreds stop at 41): the upper halves of the group
        // histograms -- phred 64-127 -- are empty, and the export below does not read them
        lo_only = fast_ok && (slow & 2u) == 0u;
        __syncthreads();
        if (!fast_ok) {
            bv_p2_row_clear<NT, RANKS, GROUPS, HALF ? 256u : 512u>(sh.hm, cx.hg, a.n_groups, tid);
            __syncthreads();
        }
    }
    if (!fast_ok) {
        bv_p2_sweep<NT, RANKS, RANKS, GROUPS>(cx, a, site, tid);
        if (RANKS) {
            uint32_t mx = (uint32_t)bv_wave_max_i32((int)cx.maxr);
            if (lane == 0) sh.maxr[wave] = mx;
        }
        __syncthreads();
    }
    return fast_ok;
}

// rank sums: MQRankSum on wave 0, ReadPosRankSum on wave 1 (wave 0 when alone), the rank window sliding across the workgroup
// (__syncthreads: not the wave form, bv_p2_wave_exact) for ranks >= BV_RPR_WIN.  fast_ok: the histograms are the perm form's --
// one window of 256 ranks, ALT counts at word 256.
template <int NT, class SH>
__device__ __forceinline__ void bv_p2_row_ranksums(const BvPass2Args &a, SH &sh, BvP2Ctx &cx, uint32_t site, bool fast_ok, unsigned long long n1,
                                                   unsigned long long n2, int tid) {
    constexpr int NW = NT / BV_WAVE;
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t maxr = 255u;
    const uint32_t alt_off = fast_ok ? 256u : (uint32_t)BV_RPR_WIN;
    if (!fast_ok) {
        maxr = 0;
        for (int w = 0; w < NW; ++w) maxr = max(maxr, sh.maxr[w]);
    }
    if (wave == 0) {
        unsigned long long below = 0, twoR = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) twoR += bv_ranksum_window(sh.hm[w * 64 + lane], sh.hm[256 + w * 64 + lane], n1 + n2, below, lane);
        double ph = bv_ranksum_phred(twoR, n1, n2);
        if (lane == 0) a.out[site].mq_ranksum = ph;
    }
    unsigned long long below = 0, twoR = 0;
    for (uint32_t win_lo = 0;; win_lo += BV_RPR_WIN) {
        if (wave == (1 % NW)) {
            // ranks beyond the row's largest classified rank hold nothing: stop at its 64-wide block
            const int nblk = (maxr < win_lo + BV_RPR_WIN) ? (int)((maxr - win_lo) >> 6) + 1 : BV_RPR_WIN / 64;
            for (int w = 0; w < nblk; ++w) twoR += bv_ranksum_window(sh.hr[w * 64 + lane], sh.hr[alt_off + w * 64 + lane], n1 + n2, below, lane);
        }
        if (maxr < win_lo + BV_RPR_WIN) break;
        // long reads: slide the window and re-tally the ranks only
        __syncthreads();
        for (int i = tid; i < 2 * BV_RPR_WIN; i += NT) sh.hr[i] = 0u;
        __syncthreads();
        cx.win_lo = win_lo + BV_RPR_WIN;
        bv_p2_sweep<NT, true, false, false>(cx, a, site, tid);
        __syncthreads();
    }
    if (wave == (1 % NW)) {
        double ph = bv_ranksum_phred(twoR, n1, n2);
        if (lane == 0) {
            a.out[site].rpr_ranksum = ph;
            atomicOr(&a.out[site].status, BV_SITE_RANKSUM);
        }
    }
}

// groups, !INLINE: one wave turns the histogram `h` of group g into an item for the group solve kernels (bv_p2g_solve16_kernel /
// bv_p2g_hard_kernel), bins straight from the histogram; its header word waits in sh.ghdr (bv_p2_site_item_kinds).
template <bool HALF, class SH>
__device__ __forceinline__ void bv_p2_group_export(const BvPass2Args &a, SH &sh, const uint32_t *h, uint32_t v, uint32_t g, bool lo_only, int lane) {
    uint32_t c[8], dpart[4], q0 = 0, cm = 0, nbv = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if ((r & 1) && lo_only) { c[r] = 0u; continue; }  // (wave-uniform: see lo_only)
        if (HALF) c[r] = (h[(((r >> 1) << 7) | ((r & 1) << 6) | lane) >> 1] >> (16 * (lane & 1))) & 0xFFFFu;
        else c[r] = h[((r >> 1) << 7) | ((r & 1) << 6) | lane];
        cm = max(cm, c[r]);
        if (!(r & 1) && __builtin_amdgcn_readfirstlane((int)c[r]) != 0) q0 |= 1u << (r >> 1);
        const bool valid = c[r] != 0u && (((r & 1) << 6) | lane) < BV_NQ_VALID;
        nbv += (uint32_t)__popcll(__ballot(valid));
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) dpart[b] = c[2 * b] + c[2 * b + 1];
    uint32_t gd[4];
    {
        const uint32_t v8[8] = {dpart[0], dpart[1], dpart[2], dpart[3], 0u, 0u, 0u, 0u};
        uint32_t t8[8];
        bv_wave_sum8_u32(v8, t8, lane);
        gd[0] = t8[0]; gd[1] = t8[1]; gd[2] = t8[2]; gd[3] = t8[3];
    }
    const uint32_t gt = gd[0] + gd[1] + gd[2] + gd[3];
    const int seen = (gd[0] != 0) + (gd[1] != 0) + (gd[2] != 0) + (gd[3] != 0);
    const bool shal = gt <= (uint32_t)BV_ORD_MAX && seen >= 2;
    const bool big = __ballot(cm > 0xFFFFu) != 0ull;
    const bool four = q0 == 0u && nbv <= (uint32_t)BV_G16_MAX_BINS && !big && a.min_af > 0.0 && !(a.flags & BV_FLAG_WAVE_SOLVER);
    uint32_t *dst = a.gitems + ((size_t)v * a.n_groups + g) * BV_P2G_ITEM_WORDS;
    if (gt != 0u) {
        uint32_t pos0 = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if ((r & 1) && lo_only) continue;
            const uint32_t code = ((uint32_t)(r >> 1) << 7) | (uint32_t)(((r & 1) << 6) | lane);
            const bool valid = c[r] != 0u && (code & 127u) < (uint32_t)BV_NQ_VALID;
            const unsigned long long m = __ballot(valid);
            const uint32_t pos = pos0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (valid) dst[8u + pos] = four ? ((code << 16) | c[r]) : ((code << 23) | c[r]);
            pos0 += (uint32_t)__popcll(m);
        }
    }
    const uint32_t hdr = gt == 0u ? 0u : (nbv | (four ? BV_P2G_PENDING : BV_P2G_HARD) | (shal ? BV_P2G_SHALLOW : 0u));
    uint32_t w = 0u;  // (word 0, the header, follows when the site's kind is known)
#pragma unroll
    for (int b = 0; b < 4; ++b) w = (lane == 1 + b) ? gd[b] : w;
    w = (lane == 5) ? q0 : w;
    if (lane >= 1 && lane < 6) dst[lane] = w;
    if (lane == 0) sh.ghdr[g] = hdr;
}

// groups, !INLINE, last: the site's items are written; which small-group solver takes them (BV_P2G_L4 / BV_P2G_L8, bv_kernels.h) is
// decided for the site -- lane g of ONE wave classifies group g (its header word: ghdr[g]) and writes the item's header.
__device__ __forceinline__ void bv_p2_site_item_kinds(const BvPass2Args &a, const uint32_t *ghdr, uint32_t v, int lane) {
    const uint32_t hdr = (uint32_t)lane < a.n_groups ? ghdr[lane] : 0u;
    const bool pend = (hdr & BV_P2G_PENDING) != 0u;
    const uint32_t nbv = hdr & 0xFFFFu;
    // (Measured, 100 k sites x 10 k samples, 8 / 16 / 32 / 64 groups: this rule 115 / 93 / 70 / 45 M sites/s; "at most 32
    // bins -> 4 lanes" per item 103 / 80 / 73 / 46, per site 109 / 80 / 73 / 46: a job whose items need eight slots per
    // lane takes three times as long as one that needs four, so 4 lanes pay only where the items fit 16 bins.)
    const uint32_t n_pend = (uint32_t)__popcll(__ballot(pend)), n_16 = (uint32_t)__popcll(__ballot(pend && nbv <= 16u));
    const bool site_l4 = 4u * n_16 >= 3u * n_pend;
    uint32_t kind = 0u;
    if (pend && site_l4 && nbv <= 32u) kind = BV_P2G_L4;
    else if (pend && nbv <= 64u) kind = BV_P2G_L8;
    if ((uint32_t)lane < a.n_groups) a.gitems[((size_t)v * a.n_groups + (uint32_t)lane) * BV_P2G_ITEM_WORDS] = hdr | kind;
}

// ------------------------------------------------------------------------------ the kernel
// HALF (with GROUPS, not INLINE; rows of at most 65,535 samples): the group histograms hold 16-bit counters, 1 KiB per group
// instead of 2 -- with 16-32 groups that is what decides how many workgroups a CU holds (32 groups: 45 KiB instead of 77).
template <int NT, bool RANKS, bool GROUPS, bool INLINE = true, bool HALF = false, bool TAG = false>
__global__ __launch_bounds__(NT) void bv_pass2_kernel(BvPass2Args a) {
    static_assert(!HALF || (GROUPS && !INLINE), "16-bit group counters: the item-exporting form only");
    constexpr uint32_t GW = HALF ? 256u : 512u;  // words of one group's histogram
    constexpr int NW = NT / BV_WAVE;
    __shared__ BvPass2Shared<NW, INLINE, RANKS> sh;
    uint32_t *hg = bv_dyn_lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n_var = a.counters[BV_CTR_VARIANTS];
    if (GROUPS && INLINE) {
        for (int i = tid; i < BV_QBINS; i += NT) {
            sh.tab_hit[i] = a.tables->hit[i];
            sh.tab_miss[i] = a.tables->miss[i];
        }
    }

    // one variant site per workgroup; surplus workgroups (the grid is sized for the worst case,
    // every site variant, because the count lives in HBM) leave at once.  No grid-stride loop:
    // see bv_pass1.hip.
    const uint32_t v = blockIdx.x;
    if (v >= n_var) return;
    const uint32_t site = a.var_list[v];
    if (a.ch != nullptr) {  // a chained launch: the segment's (biased) planes and records
        const BvChainC ch = bv_chain_const(a.ch);
        const uint32_t sg = bv_chain_seg_uniform(ch, site);
        a.bs = ch->bs[sg]; a.q = ch->q[sg]; a.mapq = ch->mapq[sg]; a.rpr = ch->rpr[sg];
        if (!a.ch_cat) { a.ref_base = ch->ref_base[sg]; a.out = ch->out[sg]; }
        if (GROUPS) a.gout = ch->gout[sg];
    }
    // ---- facts: what pass 1 decided for this site
    const bv_site_result *res = &a.out[site];
    int ref = a.ref_base[site];
    if (ref > 4) ref = 4;
    const uint32_t depth[4] = {res->depth[0], res->depth[1], res->depth[2], res->depth[3]};
    const uint2 aw = *reinterpret_cast<const uint2 *>(&res->n_alt);
    uint32_t Ltab, lut, n1, n2;
    bv_p2_site_facts(ref, depth, aw.x, aw.y, Ltab, lut, n1, n2);
    int nc;
    const int comb = bv_lrt_ref_alts(ref, res->n_alt, res->alt, nc);

    // ---- clear
    bv_p2_row_clear<NT, RANKS, GROUPS, GW>(sh.hm, hg, a.n_groups, tid);
    __syncthreads();

    // ---- tally
    BvP2Ctx cx;
    cx.hm = sh.hm; cx.hr = sh.hr; cx.hg = hg;
    cx.lut = lut; cx.win_lo = 0; cx.n_groups = a.n_groups; cx.maxr = 0; cx.half = HALF; cx.rmask = bv_rpr_rank_mask(a.rpr_tag);
    bool lo_only;
    const bool fast_ok = bv_p2_row_tally<NT, RANKS, GROUPS, HALF, TAG>(a, sh, cx, site, Ltab, n1 + n2, tid, lo_only);

    // ---- rank sums
    if (RANKS) bv_p2_row_ranksums<NT>(a, sh, cx, site, fast_ok, n1, n2, tid);

    // ---- groups: one wave per group
    if (GROUPS) {
        for (uint32_t g = wave; g < a.n_groups; g += NW) {
            const uint32_t *h = hg + g * GW;
            if (!INLINE) {
                bv_p2_group_export<HALF>(a, sh, h, v, g, lo_only, lane);
                continue;
            }
            // INLINE: the wave compacts the group's histogram into its LDS bins and solves it (bv_lrt on [REF] + alts) -- or hands it
            // over as an item where the 16-lane solver takes it.  (In the kernel's body, not a step of its own: as a function it cost
            // the INLINE instantiations 2-3 VGPRs.)
            uint32_t nb = 0, gdepth[4], gtotal = 0, q0_mask = 0;
            uint32_t cmax = 0;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int b = r >> 1;
                const int q = ((r & 1) << 6) | lane;
                uint32_t c = h[(b << 7) | q];
                cmax = max(cmax, c);
                if (!(r & 1) && __builtin_amdgcn_readfirstlane((int)c) != 0) q0_mask |= 1u << b;  // phred-0 calls of base b
                uint32_t cs = bv_wave_sum_u32(c);
                if (r & 1) gdepth[b] += cs; else gdepth[b] = cs;
                bool valid = (c != 0) && (q < BV_NQ_VALID);
                unsigned long long m = __ballot(valid);
                uint32_t pos = nb + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (valid) {
                    sh.bin_code[wave][pos] = ((uint32_t)b << 7) | (uint32_t)q;
                    sh.bin_cnt[wave][pos] = c;
                }
                nb += (uint32_t)__popcll(m);
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) gtotal += gdepth[b];
            bv_lrt_sync<0>();
            const int n_seen = (gdepth[0] != 0) + (gdepth[1] != 0) + (gdepth[2] != 0) + (gdepth[3] != 0);
            const bool shallow = gtotal <= (uint32_t)BV_ORD_MAX && n_seen >= 2;
            // The LRT of an ordinary group is a small problem (<= 128 bins) that a quarter wave solves as fast as a
            // whole one: hand it to bv_p2g_solve16_kernel (four groups per wave) and go on streaming.  Kept here: shallow
            // groups (ordered replay), phred-0 calls and min_af <= 0 (literal 0/0 arithmetic), > 128 bins, counts past 16 bits.
            const size_t item = (size_t)v * a.n_groups + g;
            if (a.gitems != nullptr && item < (size_t)a.gitem_cap) {
                uint32_t *dst = a.gitems + item * BV_P2G_ITEM_WORDS;
                const bool big = __ballot(cmax > 0xFFFFu) != 0ull;
                const bool hand_over = gtotal > 0 && !shallow && q0_mask == 0u && nb <= (uint32_t)BV_G16_MAX_BINS && !big && a.min_af > 0.0 &&
                                       !(a.flags & BV_FLAG_WAVE_SOLVER);
                if (lane == 0) {
                    dst[0] = hand_over ? (nb | BV_P2G_PENDING) : 0u;
                    dst[1] = gdepth[0]; dst[2] = gdepth[1]; dst[3] = gdepth[2]; dst[4] = gdepth[3]; dst[5] = q0_mask;
                }
                if (hand_over) {
                    for (uint32_t i = (uint32_t)lane; i < nb; i += BV_WAVE) dst[8u + i] = (sh.bin_code[wave][i] << 16) | sh.bin_cnt[wave][i];
                    bv_lrt_sync<0>();
                    continue;
                }
            }
            BvLrtOut L;
            L.n_alt = 0; L.alt_packed = 0; L.af[0] = L.af[1] = L.af[2] = L.af[3] = 0.;
            if (gtotal > 0) {
                BvBins B;
                B.code = sh.bin_code[wave]; B.cnt = sh.bin_cnt[wave]; B.skip_mask = 0u;
                B.hit = sh.tab_hit; B.miss = sh.tab_miss; B.nb = (int)nb;
                B.loghit = a.tables->loghit; B.logmiss = a.tables->logmiss; B.ord = nullptr; B.n_ord = 0;
                if (shallow) {
                    // a shallow group with more than one base: the reference's per-sample order decides ties (bv_em_ordered)
                    const uint32_t got = bv_gather_ordered(a.bs + (size_t)site * a.pitch, a.q + (size_t)site * a.pitch,
                                                           a.n_samples, sh.ord[wave], lane, a.group_id, g);
                    bv_lrt_sync<0>();
                    if (got == gtotal) { B.ord = sh.ord[wave]; B.n_ord = (int)gtotal; }
                }
                bv_lrt<0>(B, gdepth, gtotal, comb, nc, ref, a.min_af, &sh.lrt[wave], wave, lane, L, q0_mask);
            }
            if (lane == 0) {
                bv_group_result gr;
                gr.n_alt = (uint8_t)L.n_alt;
                gr.reserved[0] = gr.reserved[1] = gr.reserved[2] = 0;
                gr.total_depth = gtotal;
                gr.reserved2 = 0;
#pragma unroll
                for (int k = 0; k < BV_MAX_ALT; ++k) {
                    gr.alt[k] = (k < L.n_alt) ? (uint8_t)bv_alt_at(L, k) : 0;
                    gr.af[k] = (k < L.n_alt) ? L.af[k] : 0.0;
                }
                a.gout[(size_t)site * a.n_groups + g] = gr;
            }
            bv_lrt_sync<0>();
        }
        if (!INLINE) {
            __syncthreads();
            if (wave == 0) bv_p2_site_item_kinds(a, sh.ghdr, v, lane);
        }
    }
}
