// bv_pass2.hip -- pass 2 of the per-site basetype path: variant sites only.
//
// For every site that pass 1 flagged BV_SITE_VARIANT (index list in HBM, no host round
// trip) one workgroup re-reads the row's call plane together with the planes that only the
// VCF record needs, and finishes the record:
//   MQRankSum, ReadPosRankSum    ref_vs_alt_ranksumtest, src/basetype.cpp:201-233 via
//                                caller.cpp:1151-1154 (values are small integers, so the
//                                Wilcoxon statistic is computed from per-class histograms)
//   <group>_AF                   __gb(): BaseType(subset) + lrt([REF]+alts),
//                                caller.cpp:756-759, 767-797 -- one (base x phred)
//                                histogram per pop-group, each solved by one wave
// Traffic: 1 B (calls) + 1 B (mapq) + 2 B (rpr) per cell, + 1 B (phred) when groups exist;
// the group-id vector is shared by all sites and stays in L2.
#include "bv_kernels.h"
#include "bv_tally.h"
#include "bv_pass2_sweep.h"  // BvP2Ctx, bv_p2_sweep, bv_p2_site_facts, bv_p2_wave_exact, BV_RPR_WIN
#include "bv_pass2_row.h"   // BvPass2Shared, bv_p2_fast_sweep, bv_pass2_kernel
#include "bv_pass2_wave.h"  // bv_pass2_short_kernel, bv_pass2_dma_kernel, BV_P2S_WAVES, BV_P2D_WAVES

#define BV_P2_WIDE_GROUPS 2 /* from this many pop-groups on, short rows also take the four-wave kernel: one wave per group */
#define BV_P2_BIG_GROUPS 12 /* from this many pop-groups on, long rows take workgroups of eight waves */

size_t bv_pass2_lds_bytes(uint32_t n_groups) { return (size_t)n_groups * 512u * sizeof(uint32_t); }

template <int NT>
static void bv_launch_pass2_nt(const BvPass2Args &a, hipStream_t stream) {
    const bool ranks = a.mapq != nullptr && a.rpr != nullptr;
    const bool groups = a.n_groups > 0 && a.group_id != nullptr && a.gout != nullptr;
    if (!ranks && !groups) return;
    uint32_t grid = a.n_sites;
    size_t dyn = groups ? bv_pass2_lds_bytes(a.n_groups) : 0;
    const bool items = bv_p2g_all_items(a);
    // many groups on rows whose counts fit 16 bits: half the histogram, more workgroups per CU -- from 14 groups on, where 32-bit
    // counters leave room for three workgroups (13 KiB + 2 KiB per group of 160); below that the three extra VALU per cell cost
    // more than the occupancy brings (100 k sites x 10 k samples: 8 groups -3 %, 12 +-0, 14 +4 %, 16 +4.5 %, 32 +9 %)
    if (NT == 256 && groups && items && a.n_groups >= 14u && a.n_samples <= 65535u) {
        dyn /= 2;
        if (ranks) hipLaunchKernelGGL((bv_pass2_kernel<256, true, true, false, true>), dim3(grid), dim3(256), dyn, stream, a);
        else hipLaunchKernelGGL((bv_pass2_kernel<256, false, true, false, true>), dim3(grid), dim3(256), dyn, stream, a);
        return;
    }
    if (ranks && groups && items)
        hipLaunchKernelGGL((bv_pass2_kernel<NT, true, true, false>), dim3(grid), dim3(NT), dyn, stream, a);
    else if (ranks && groups)
        hipLaunchKernelGGL((bv_pass2_kernel<NT, true, true, true>), dim3(grid), dim3(NT), dyn, stream, a);
    else if (ranks && a.rpr_tag)
        hipLaunchKernelGGL((bv_pass2_kernel<NT, true, false, true, false, true>), dim3(grid), dim3(NT), dyn, stream, a);
    else if (ranks)
        hipLaunchKernelGGL((bv_pass2_kernel<NT, true, false>), dim3(grid), dim3(NT), dyn, stream, a);
    else if (items)
        hipLaunchKernelGGL((bv_pass2_kernel<NT, false, true, false>), dim3(grid), dim3(NT), dyn, stream, a);
    else
        hipLaunchKernelGGL((bv_pass2_kernel<NT, false, true, true>), dim3(grid), dim3(NT), dyn, stream, a);
}

void bv_launch_pass2(const BvPass2Args &a_in, hipStream_t stream) {
    BvPass2Args a = a_in;
    const bool ranks = a.mapq != nullptr && a.rpr != nullptr;
    bool groups = a.n_groups > 0 && a.group_id != nullptr && a.gout != nullptr;
    if (bv_p2g_streams(a)) {
        // short rows with pop-groups: the group tallies stream on their own (2 B per cell), the rank sums below as if
        // there were no groups (4 B per cell); the items are solved by bv_launch_p2g_solve16
        bv_launch_p2g_stream(a, stream);
        groups = false;
        a.n_groups = 0; a.group_id = nullptr; a.gout = nullptr;
        if (!ranks) return;
    }
    if (a.n_samples > 2048u && a.n_samples <= BV_SHORT_ROW_MAX && ranks && !groups && !(a.flags & BV_FLAG_PASS2_SWEEP)) {
        uint32_t grid = (a.n_cu ? a.n_cu : 256u) * 2u;  // 64 KiB of LDS per workgroup: 2 per CU, 8 waves
        const uint32_t need = (a.n_sites + BV_P2D_WAVES - 1) / BV_P2D_WAVES;
        if (grid > need) grid = need;
        const uint32_t cap = (a.flags >> 16) & 0xFFu;  // BV_FLAG_GRID_LIMIT
        if (cap && grid > cap) grid = cap;
        if (a.rpr_tag) hipLaunchKernelGGL(bv_pass2_dma_kernel<true>, dim3(grid), dim3(BV_WAVE * BV_P2D_WAVES), 0, stream, a);
        else hipLaunchKernelGGL(bv_pass2_dma_kernel<false>, dim3(grid), dim3(BV_WAVE * BV_P2D_WAVES), 0, stream, a);
        return;
    }
    if (a.n_samples <= 16384u && ranks && !groups) {
        uint32_t grid = (a.n_cu ? a.n_cu : 256u) * 4u;  // 16 KiB of LDS and <= 128 VGPRs: 4 workgroups per CU
        const uint32_t need = (a.n_sites + BV_P2S_WAVES - 1) / BV_P2S_WAVES;
        if (grid > need) grid = need;
        hipLaunchKernelGGL(bv_pass2_short_kernel, dim3(grid), dim3(BV_WAVE * BV_P2S_WAVES), 0, stream, a);
        return;
    }
    if (a.n_samples <= 16384u && !(groups && a.n_groups >= BV_P2_WIDE_GROUPS)) bv_launch_pass2_nt<64>(a, stream);
    // many pop-groups: 2 KiB of histogram per group leave room for two workgroups per CU only -- eight waves each then
    // (sixteen waves were measured too: 10 % slower than eight at 24-32 groups)
    else if (groups && a.n_groups >= BV_P2_BIG_GROUPS && bv_p2g_all_items(a) && a.n_samples > 16384u) bv_launch_pass2_nt<512>(a, stream);
    else bv_launch_pass2_nt<256>(a, stream);
}
