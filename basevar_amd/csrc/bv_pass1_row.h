// bv_pass1_row.h -- how one tally wave of the long-row kernel streams its share of a row: two register sets of BV_TALLY_U
// chunks per plane, software-pipelined, tallied into the slot's histogram (bv_tally_chunk, bv_tally.h).
// Included by bv_pass1.hip alone; bv_pass1_kernel calls bv_tally_row_wave.
#pragma once

#include "bv_kernels.h"
#include "bv_tally.h"

// One wave streams one row, software-pipelined: two register sets of U chunks per plane, the
// loads of the next set are in flight (16 KiB per wave) while the current set is tallied.
#define BV_TALLY_U 4
struct BvChunkSet {
    bv_u32x4 vb[BV_TALLY_U], vq[BV_TALLY_U];
};
// FULL: every chunk of the set lies wholly inside the row (wave-uniform fact) -- unguarded loads off a
// scalar base (row pointer + set offset in SGPRs, lane offset in one VGPR, the chunk's 1 KiB step in
// the instruction's immediate) and no tail masking.  !FULL: the row's last, partial set.
template <bool FULL>
__device__ __forceinline__ void bv_chunks_load(BvChunkSet &c, const uint8_t *bs_row, const uint8_t *q_row, uint32_t base,
                                               uint32_t n_chunks, int lane) {
    const uint8_t *pb = bs_row + (size_t)base * 16u, *pq = q_row + (size_t)base * 16u;  // uniform
    const uint32_t voff = (uint32_t)lane * 16u;
#pragma unroll
    for (int u = 0; u < BV_TALLY_U; ++u) {
        const uint32_t off = voff + (uint32_t)u * (BV_WAVE * 16u);
        if (FULL || base + u * BV_WAVE + lane < n_chunks) {
            c.vb[u] = __builtin_nontemporal_load(reinterpret_cast<const bv_u32x4 *>(pb + off));
            c.vq[u] = __builtin_nontemporal_load(reinterpret_cast<const bv_u32x4 *>(pq + off));
        } else {
            c.vb[u] = bv_u32x4{0x08080808u, 0x08080808u, 0x08080808u, 0x08080808u};
            c.vq[u] = bv_u32x4{0u, 0u, 0u, 0u};
        }
    }
}
template <bool FULL, bool SWZ>
__device__ __forceinline__ void bv_chunks_tally(BvChunkSet &c, uint32_t base, uint32_t n_chunks, int tail, int lane,
                                                uint32_t *hist, uint32_t one) {
#pragma unroll
    for (int u = 0; u < BV_TALLY_U; ++u) {
        if (!FULL) {
            uint32_t idx = base + u * BV_WAVE + lane;
            if (tail && idx == n_chunks - 1) {
                c.vb[u].x = bv_mask_tail_dword(c.vb[u].x, tail);
                c.vb[u].y = bv_mask_tail_dword(c.vb[u].y, tail - 4);
                c.vb[u].z = bv_mask_tail_dword(c.vb[u].z, tail - 8);
                c.vb[u].w = bv_mask_tail_dword(c.vb[u].w, tail - 12);
            }
        }
        bv_tally_chunk<2, SWZ>(c.vb[u], c.vq[u], hist, one);
    }
}
// set at `base`: nothing to do past the row's end; FULL form when the set ends inside the row
#define BV_SET_LOAD(C, BASE)                                                                  \
    do {                                                                                      \
        const uint32_t b_ = (BASE);                                                           \
        if (b_ + BLK <= n_full) bv_chunks_load<true>(C, bs_row, q_row, b_, n_chunks, lane);   \
        else if (b_ < n_chunks) bv_chunks_load<false>(C, bs_row, q_row, b_, n_chunks, lane);  \
    } while (0)
#define BV_SET_TALLY(C, BASE)                                                                 \
    do {                                                                                      \
        const uint32_t b_ = (BASE);                                                           \
        if (b_ + BLK <= n_full) bv_chunks_tally<true, SWZ>(C, b_, n_chunks, tail, lane, hist, one);\
        else if (b_ < n_chunks) bv_chunks_tally<false, SWZ>(C, b_, n_chunks, tail, lane, hist, one);\
    } while (0)
// wave t of the NTALLY that share the row; SWZ: with the dense-row bank swizzle
template <int NTALLY, bool SWZ>
__device__ __forceinline__ void bv_tally_row_wave(const uint8_t *bs_row, const uint8_t *q_row, uint32_t n_samples,
                                                  uint32_t *hist, int t, int lane) {
    const uint32_t n_chunks = (n_samples + 15u) >> 4, n_full = n_samples >> 4;
    const int tail = (int)(n_samples & 15u);
    constexpr uint32_t BLK = BV_WAVE * BV_TALLY_U;  // chunks per wave-iteration (4 KiB of each plane)
    constexpr uint32_t STRIDE = BLK * NTALLY;       // the row's blocks go round-robin over the tally waves
    uint32_t one;
    asm volatile("v_mov_b32 %0, 1" : "=v"(one));  // opaque: not re-materialised per cell
    BvChunkSet A, B;
    uint32_t base = (uint32_t)t * BLK;
    BV_SET_LOAD(A, base);
    for (; base < n_chunks; base += 2 * STRIDE) {
        BV_SET_LOAD(B, base + STRIDE);
        BV_SET_TALLY(A, base);
        BV_SET_LOAD(A, base + 2 * STRIDE);
        BV_SET_TALLY(B, base + STRIDE);
    }
}
#undef BV_SET_LOAD
#undef BV_SET_TALLY
