// bv_text_image.h -- what a kernel needs that writes text one wave per (row, tile) (bv_vcf.hip, bv_pileup_text.hip): the tile of a
// workgroup, the tile's plane rows, wave sums, the head copy by tile 0, and the LDS image of a piece of the text with its store.
// The image is laid out as the text is modulo 16, so that it goes out with 16-byte stores over the aligned interior and byte stores
// on the at most 15 bytes at each edge: neighbouring pieces share 16-byte words, and every byte of the text has exactly one writer.
// That cut is bv_span_words, plain integer code that a CPU check compiles alone (tests/cpp/text_image_check.cpp); the rest is
// device code.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BV_TEXT_IMAGE_FN __host__ __device__ __forceinline__
#else
#define BV_TEXT_IMAGE_FN inline
#endif

// The image range [lo, hi) cut at the 16-byte words: bytes [lo, lead_end), the whole words [w_lo, w_hi) (empty where
// w_hi <= w_lo: no whole word lies inside), bytes [tail_at, hi)
struct BvSpanWords {
    uint32_t lead_end, w_lo, w_hi, tail_at;
};

BV_TEXT_IMAGE_FN BvSpanWords bv_span_words(uint32_t lo, uint32_t hi) {
    BvSpanWords s;
    s.w_lo = (lo + 15u) / 16u;
    s.w_hi = hi / 16u;
    s.lead_end = 16u * s.w_lo < hi ? 16u * s.w_lo : hi;
    s.tail_at = 16u * s.w_hi > s.lead_end ? 16u * s.w_hi : s.lead_end;
    return s;
}

#if defined(__HIPCC__)
namespace bv_impl {

// The (row, tile) of this workgroup and the tile's samples, for rows cut into tiles of `tile_samples`
struct TileOfBlock {
    uint32_t k, tile, cnt;
};

__device__ __forceinline__ TileOfBlock tile_of_block(uint32_t n_tiles, uint32_t n_samples, uint32_t tile_samples) {
    const uint32_t tile = blockIdx.x % n_tiles;
    return {blockIdx.x / n_tiles, tile, min(tile_samples, n_samples - tile * tile_samples)};
}

// the lane's 16 bytes of a tile's plane row, which begins at `p`, or zeros where the tile has no sample there
__device__ __forceinline__ uint4 tile_load16(const uint8_t *p, uint32_t cnt, uint32_t lane) {
    if (16u * lane >= cnt) return make_uint4(0, 0, 0, 0);
    return *reinterpret_cast<const uint4 *>(p + 16u * lane);
}

// the same for a plane of uint16: the lane's 16 cells are two loads
__device__ __forceinline__ void tile_load16x2(const uint16_t *p, uint32_t cnt, uint32_t lane, uint4 *dst) {
    const bool in = 16u * lane < cnt;
    dst[0] = in ? *reinterpret_cast<const uint4 *>(p + 16u * lane) : make_uint4(0, 0, 0, 0);
    dst[1] = in ? *reinterpret_cast<const uint4 *>(p + 16u * lane + 8u) : make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
    return v;
}

// inclusive prefix sum over the lanes; lane 63 holds the wave's sum
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// tile 0 copies the row's head
__device__ __forceinline__ void head_copy(uint8_t *dst, const uint8_t *head, uint64_t bytes, uint32_t lane) {
    for (uint64_t i = lane; i < bytes; i += 64u) dst[i] = head[i];
}

// A piece of the text under construction: image[i] is the byte of the text at g + i, and g is 16-byte aligned.  The piece owns
// image [lo, fill); `left` bytes of the text are the piece's to write, whatever the planes say by now.  All of it is wave-uniform.
struct Piece {
    uint8_t *g;
    uint32_t lo, fill;
    uint64_t left;
};

__device__ __forceinline__ void piece_open(Piece &p, uint8_t *text, uint64_t dst, uint64_t bytes) {
    const uint32_t shift = (uint32_t)(dst & 15u);
    p.g = text + (dst - shift);
    p.lo = p.fill = shift;
    p.left = bytes;
}

// Store the piece's bytes: all of them (last), or its whole 16-byte words, the rest moving to the image's front.
__device__ __forceinline__ void piece_flush(Piece &p, uint8_t *image, bool last, uint32_t lane) {
    __syncthreads();
    const uint32_t lo = p.lo, hi = lo + (uint32_t)min((uint64_t)(p.fill - lo), p.left);
    const BvSpanWords s = bv_span_words(lo, hi);
    if (last) {
        for (uint32_t i = lo + lane; i < s.lead_end; i += 64u) p.g[i] = image[i];
        for (uint32_t w = s.w_lo + lane; w < s.w_hi; w += 64u) reinterpret_cast<uint4 *>(p.g)[w] = reinterpret_cast<const uint4 *>(image)[w];
        for (uint32_t i = s.tail_at + lane; i < hi; i += 64u) p.g[i] = image[i];
        p.left -= hi - lo;
        p.lo = p.fill = hi;
        return;
    }
    const uint32_t cut = 16u * s.w_hi;  // the last word boundary inside the piece
    if (cut <= lo) { p.fill = hi; return; }
    for (uint32_t i = lo + lane; i < s.lead_end; i += 64u) p.g[i] = image[i];
    for (uint32_t w = s.w_lo + lane; w < s.w_hi; w += 64u) reinterpret_cast<uint4 *>(p.g)[w] = reinterpret_cast<const uint4 *>(image)[w];
    const uint32_t keep = hi - cut;  // < 16
    const uint8_t v = lane < keep ? image[cut + lane] : (uint8_t)0;
    __syncthreads();
    if (lane < keep) image[lane] = v;
    p.g += cut;
    p.left -= cut - lo;
    p.lo = 0; p.fill = keep;
    __syncthreads();
}

}  // namespace bv_impl
#endif  // __HIPCC__
