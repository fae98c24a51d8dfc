// bv_pass1_short.hip -- pass 1 for short rows (<= 49,152 samples per site) as two kernels: a streaming kernel
// (bv_short_stream.h) and a solve kernel (bv_short_solve.h).  This file keeps their launchers and the gather / scatter kernels
// of chained launches.  Rows of at most 4,096 samples take this form (and BV_FLAG_SHORT_ROW_FORM(9) in the tests); longer
// short rows take the fused kernel (bv_pass1_fused.hip), which shares the steps in bv_short.h.
//
// On short rows the solve, not the stream, used to set the pace of pass 1: one wave tallied a row and then solved it,
// and while it solved nothing of its own was in flight (40-51 % of the HBM peak at 10 k samples).  Here the two
// halves are separate kernels that meet in a small HBM scratch:
//
//   bv_p1s_stream_kernel   a WORKGROUP owns a contiguous range of sites; its waves draw chunks of consecutive sites from a
//                          cursor in LDS, and every wave streams the rows of its chunks as ONE sequence of slots (64 lanes
//                          x 16 bytes x U of the call plane, then of the phred plane) through a private ring in LDS filled
//                          by LDS-DMA (global_load_lds_dwordx4: no VGPRs, no wait until the slot is consumed, K slots in
//                          flight per wave ACROSS row and chunk boundaries -- the next rows are already on their way while
//                          a row's totals are formed).  Per site it leaves a 48-byte
//                          summary (strand x base totals, flags); only sites that need the EM -- more than one active
//                          base, a non-reference base, a phred-0 call, a deep strand table -- also export their
//                          compacted (base, phred) bins and go on one of the candidate lists.
//   bv_p1s_solve16_kernel  (a) the candidates only the wave solver takes (shallow sites, phred-0 calls, > 128 bins) get a whole
//                          wave and the full solver of bv_solver.h on their bins; (b) the ordinary candidates are solved four
//                          per wave, one per group of 16 lanes (bv_solver16.h); (c) every non-candidate site (hom-ref, or
//                          uncovered) is finished ONE LANE PER SITE: the work there is scalar per site (depths, one small
//                          Fisher test), and a whole wave per site repeated it 64 times over.
//
// Reference functions realised: those of bv_pass1.hip (src/basetype.cpp:22-295, src/algorithm.h:44-255,
// htslib/kfunc.c:39-143,197-313); results are bit-identical to the one-kernel form for candidates (same bins, same
// order, same solver) and equal to ~1e-13 relative for the per-lane Fisher test, which walks the tables exactly as
// kt_fisher_exact does (kfunc.c:291-307, incremental hypergeo_acc with its re-seeding every 11 tables).
//
// HBM-bound by design (2 B per cell, each byte read once); no MFMA (categorical tallies).
#define BV_LNFACT_TABLE_ONLY 1  /* rows of at most 65,535 samples: see bv_lnfact */
#include "bv_kernels.h"

#include "bv_solver.h"
#include "bv_solver16.h"
#include "bv_tally.h"

#include "bv_short.h"

#include "bv_short_stream.h"
#include "bv_short_solve.h"

// ------------------------------------------------------------------------------ chained launches (bv_engine_submit_many)
__global__ void bv_chain_gather_ref_kernel(const BvChain *ch, uint32_t n_sites, uint8_t *ref_cat) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const BvChainC c = bv_chain_const(ch);
    if (t < n_sites) ref_cat[t] = c->ref_base[bv_chain_seg(c, t)][t];
}
// one 16-byte piece of a record per thread (13 per record)
__global__ void bv_chain_scatter_out_kernel(const BvChain *ch, uint32_t n_sites, const bv_site_result *out_cat) {
    constexpr uint32_t PIECES = (uint32_t)(sizeof(bv_site_result) / 16);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t t = (uint32_t)(i / PIECES), piece = (uint32_t)(i % PIECES);
    const BvChainC c = bv_chain_const(ch);
    if (t < n_sites)
        reinterpret_cast<uint4 *>(&c->out[bv_chain_seg(c, t)][t])[piece] = reinterpret_cast<const uint4 *>(&out_cat[t])[piece];
}
void bv_launch_chain_gather_ref(const BvChain *ch, uint32_t n_sites, uint8_t *ref_cat, hipStream_t stream) {
    hipLaunchKernelGGL(bv_chain_gather_ref_kernel, dim3((n_sites + 255u) / 256u), dim3(256), 0, stream, ch, n_sites, ref_cat);
}
void bv_launch_chain_scatter_out(const BvChain *ch, uint32_t n_sites, const bv_site_result *out_cat, hipStream_t stream) {
    const uint64_t n = (uint64_t)n_sites * (sizeof(bv_site_result) / 16);
    hipLaunchKernelGGL(bv_chain_scatter_out_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, ch, n_sites, out_cat);
}

// ------------------------------------------------------------------------------ launchers
template <int NW, int K, int U>
static void bv_launch_p1s_stream_cfg(const BvP1ShortArgs &a, hipStream_t stream) {
    uint32_t grid = a.n_cu ? a.n_cu : 256u;  // one workgroup per CU
    const uint32_t need = (a.n_sites + NW - 1) / NW;  // at least one site per wave
    if (grid > need) grid = need > 0 ? need : 1;
    const uint32_t cap = (a.flags >> 16) & 0xFFu;  // BV_FLAG_GRID_LIMIT
    if (cap && grid > cap) grid = cap;
    if (a.ch != nullptr) hipLaunchKernelGGL((bv_p1s_stream_kernel<NW, K, U, true>), dim3(grid), dim3(BV_WAVE * NW), 0, stream, a);
    else hipLaunchKernelGGL((bv_p1s_stream_kernel<NW, K, U, false>), dim3(grid), dim3(BV_WAVE * NW), 0, stream, a);
}
void bv_launch_p1s_stream(const BvP1ShortArgs &a, hipStream_t stream) {
    // (Measured and dropped, rounds 2-3: 16 waves / CU with 2 slots in flight, 8 with 5, two workgroups of 4 waves, 6 or 5 waves
    // per workgroup, slots of 1 KiB per plane at 8 or 12 waves / CU.)
    // Slots of 2 KiB per plane, 3 slots per wave (8 KiB in flight), 8 waves per CU: measured best (+4-5 % over 1 KiB
    // slots; 4 slots of 2 KiB or 8 of 1 KiB need 82 KB of LDS per workgroup -- one workgroup per CU, 0.43 of peak)
    // One workgroup of 8 waves per CU (not two of 4): the waves of a workgroup share its sites through the LDS cursor, and the
    // two waves that share a SIMD -- the arbiter's favourite and the other -- must be in the same workgroup for that to even
    // them out.
    // (Also under BV_FLAG_LANES, where the other lane's kernels run beside this one.  Measured there, interleaved A/B: this
    // shape 170.5 M sites/s, two workgroups of 4 waves with fixed ranges 167-171 M, two of 4 with the cursor 157 M; 176-178 M
    // since the wave-solver candidates moved into the solve kernel: DESIGN 4.2c.)
    bv_launch_p1s_stream_cfg<8, 3, 2>(a, stream);
}
// `beside_stream`: the kernels will run beside a streaming kernel (the next chunk's pass 1 or an earlier chunk's pass 2) whose
// two workgroups per CU leave 28-32 KB of LDS: grids of ONE workgroup per CU then -- with more, whatever starts in the
// gap between two streaming kernels takes the LDS of a streaming workgroup for its whole (persistent) life.
void bv_launch_p1s_solve(const BvP1ShortArgs &a, hipStream_t stream, bool beside_stream) {
    const uint32_t cu = a.n_cu ? a.n_cu : 256u;
    const uint32_t cap = (a.flags >> 16) & 0xFFu;  // BV_FLAG_GRID_LIMIT
    uint32_t grid16 = beside_stream ? cu : cu * (uint32_t)BV_P1S_SOLVE16_OCC * (4u / BV_P1S_SOLVE16_NW);
    const uint32_t need16 = (a.n_sites + 4 * BV_P1S_SOLVE16_NW - 1) / (4 * BV_P1S_SOLVE16_NW);  // four sites per wave
    if (grid16 > need16) grid16 = need16 > 0 ? need16 : 1;
    if (cap && grid16 > cap) grid16 = cap;
    hipLaunchKernelGGL(bv_p1s_solve16_kernel, dim3(grid16), dim3(BV_WAVE * BV_P1S_SOLVE16_NW), 0, stream, a);
}
