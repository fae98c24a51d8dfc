// bv_pileup_text_impl.h -- what the two schedules of the batchfile row writer share: bv_pileup_text.hip (rows of a whole tile)
// and bv_pileup_text_parts.hip (rows over sample parts of it).  The device part -- the kernels' arguments, the tile's plane rows
// in LDS and the list writer -- is in an unnamed namespace: each file's kernels inline their own copy.  The host part is the
// per-engine state, the resolved tile of a call, its checks and its planes, defined in bv_pileup_text.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/basevar_amd_pileup_text.h"
#include "bv_chunk_stage.h"
#include "bv_device_text.h"
#include "bv_pileup_core.h"
#include "bv_pileup_text_core.h"
#include "bv_text_image.h"

using namespace bv_impl;

namespace {

// Samples of a tile: one 16-byte load a lane and byte plane.  The write kernel's LDS is the tile's four plane rows (5 KiB) and
// the image (4 KiB): seventeen workgroups fit a CU's 160 KiB.
constexpr uint32_t BV_PTEXT_TILE = 1024;
constexpr uint32_t kImage = 4096;
constexpr uint32_t kNoSample = 0xffffffffu;
static_assert(BV_PTEXT_TILE == 64u * 16u, "a lane loads 16 cells of a tile");
static_assert(kImage % 16u == 0 && kImage >= 64u * 6u + 32u, "a step of ranks fits the image behind a flush");

struct PtextArgs {
    const uint8_t *cell, *qual, *mapq;  // [.][pitch], 16-byte aligned rows; row k of the call is plane row row0 + k
    const uint16_t *rank;
    uint64_t pitch;
    const BvPtextToken *tokens;         // the tokens of the call's rows, ascending by (pos, sample)
    uint64_t n_tokens;
    const uint8_t *tok_text;            // token t's text is tok_text[text_off ..)
    const uint8_t *head;
    const uint64_t *head_off;           // [n_rows + 1]
    const uint64_t *row_off;            // [n_rows + 1] (write kernel)
    uint4 *tile_sum;                    // [n_rows][n_tiles]: token bytes of M, B, R in the tile and its first sample without a
                                        // token (kNoSample: none); after the scan x, y, z are those of the tiles before it
    uint4 *row_sum;                     // [n_rows]: the row's
    uint8_t *text;
    uint32_t row0, pos0, n_rows, n_samples, n_tiles;
};

struct TileRows {
    uint8_t cell[BV_PTEXT_TILE], qual[BV_PTEXT_TILE], mapq[BV_PTEXT_TILE];
    uint16_t rank[BV_PTEXT_TILE];
};

// the tile's piece of the four plane rows to LDS; lanes beyond the tile's samples store zeros (rank 0: never looked at anyway)
__device__ __forceinline__ void tile_stage(TileRows *t, const PtextArgs &a, uint32_t k, uint32_t tile, uint32_t cnt, uint32_t lane) {
    const size_t at = (size_t)(a.row0 + k) * a.pitch + (size_t)tile * BV_PTEXT_TILE;
    reinterpret_cast<uint4 *>(t->cell)[lane] = tile_load16(a.cell + at, cnt, lane);
    reinterpret_cast<uint4 *>(t->qual)[lane] = tile_load16(a.qual + at, cnt, lane);
    reinterpret_cast<uint4 *>(t->mapq)[lane] = tile_load16(a.mapq + at, cnt, lane);
    tile_load16x2(a.rank + at, cnt, lane, reinterpret_cast<uint4 *>(t->rank) + 2u * lane);
}


// One list of the tile: LIST 0 .. 4 = M B Q R S
template <uint32_t LIST>
__device__ __forceinline__ void write_list(const PtextArgs &a, const TileRows &rows, uint8_t *image, uint64_t dst, uint64_t bytes, uint32_t tile, uint32_t cnt,
                                  uint32_t pos, uint32_t lane) {
    Piece p;
    piece_open(p, a.text, dst, bytes);
    for (uint32_t s0 = 0; s0 < cnt; s0 += 64u) {
        const uint32_t s = s0 + lane, n_act = min(64u, cnt - s0), sample = tile * BV_PTEXT_TILE + s;
        const bool active = s < cnt;
        const uint32_t rk = active ? rows.rank[s] : 0u;
        const uint8_t c = active ? rows.cell[s] : (uint8_t)0;
        const uint8_t sep = bv_ptext_sep(LIST, sample, a.n_samples);
        const uint64_t any = __ballot(rk != 0u);
        uint32_t len = 1, at = 2u * lane, total = 2u * n_act;  // the token's bytes, its place behind the step's base, the step's bytes
        uint32_t value = 0;       // M, R: the number; B, Q, S: the character
        uint64_t tok_off = 0;     // B: an indel token's text
        bool is_tok = false;
        if (LIST == 0) value = rk ? rows.mapq[s] : 0u;
        else if (LIST == 1) value = rk ? bv_ptext_base_char(c) : (uint8_t)'N';
        else if (LIST == 2) value = rk ? bv_ptext_qual_char(rows.qual[s]) : (uint8_t)'!';
        else if (LIST == 3) value = rk;
        else value = rk ? bv_ptext_strand_char(c) : (uint8_t)'.';
        if (any != 0ull && (LIST == 0 || LIST == 1 || LIST == 3)) {
            if (LIST == 0 || LIST == 3) len = bv_ptext_digits(value);
            if (LIST == 1 && rk && bv_ptext_is_indel(c)) {
                const uint64_t t = bv_ptext_find(a.tokens, a.n_tokens, pos, sample);
                if (t != a.n_tokens) { is_tok = true; len = a.tokens[t].text_len; tok_off = a.tokens[t].text_off; }  // (the count pass refused the row otherwise)
            }
            const uint32_t mine = active ? len + 1u : 0u, incl = wave_incl_scan(mine, lane);
            at = incl - mine;
            total = __shfl(incl, 63, 64);
        }
        if (p.fill + total > kImage) piece_flush(p, image, false, lane);
        if (p.fill + total <= kImage) {
            if (active) {
                uint8_t *o = image + p.fill + at;
                if (LIST == 0 || LIST == 3) bv_ptext_dec(value, o);
                else if (LIST == 1 && is_tok) for (uint32_t i = 0; i < len; ++i) o[i] = a.tok_text[tok_off + i];
                else o[0] = (uint8_t)value;
                o[len] = sep;
            }
            p.fill += total;
        } else if (LIST == 1) {
            // tokens longer than the image can take in one step: sample by sample, the wave across the token's bytes
            for (uint32_t j = 0; j < n_act; ++j) {
                const uint32_t l1 = (uint32_t)__shfl(len, j, 64) + 1u, ch = __shfl(value, j, 64), sp = __shfl((uint32_t)sep, j, 64);
                const bool tk = __shfl((int)is_tok, j, 64) != 0;
                const uint64_t off = ((uint64_t)(uint32_t)__shfl((uint32_t)(tok_off >> 32), j, 64) << 32) | (uint32_t)__shfl((uint32_t)tok_off, j, 64);
                for (uint32_t done = 0; done < l1;) {
                    if (p.fill == kImage) {
                        const uint32_t before = p.fill;
                        piece_flush(p, image, false, lane);
                        if (p.fill == before) return;  // (the piece has no bytes left to write: cannot happen behind the count pass)
                        continue;
                    }
                    const uint32_t take = min(kImage - p.fill, l1 - done);
                    for (uint32_t i = lane; i < take; i += 64u) {
                        const uint32_t idx = done + i;
                        image[p.fill + i] = idx + 1u == l1 ? (uint8_t)sp : tk ? a.tok_text[off + idx] : (uint8_t)ch;
                    }
                    p.fill += take;
                    done += take;
                }
            }
        }
    }
    piece_flush(p, image, true, lane);
    __syncthreads();
}


}  // namespace

// Per-engine state of bv_engine_pileup_text: the formatted text and what the kernels read beside the planes.
struct BvPtextState {
    DeviceText text;             // the formatted rows
    uint8_t *d_tok = nullptr;    // the tokens of the call's rows; behind them an explicit tile's token text
    uint8_t *d_head = nullptr;   // head_off u64 [n + 1], row_off u64 [n + 1], the heads
    uint8_t *d_sum = nullptr;    // tile_sum uint4 [n][tiles], row_sum uint4 [n], depth + max_rank u32 [2 n], ref bytes [n]
    uint8_t *d_rows = nullptr;   // an explicit tile's rows of the call, packed: cell, qual, mapq [n][P], rank [n][P]
    size_t tok_cap = 0, head_cap = 0, sum_cap = 0, rows_cap = 0;
};

namespace bv_impl {

// the tile of a call, resolved: device planes of the engine's pileup, or an explicit tile's host / device planes
struct TileView {
    const uint8_t *cell = nullptr, *qual = nullptr, *mapq = nullptr;
    const uint16_t *rank = nullptr;
    uint64_t pitch = 0;
    uint32_t rows = 0, n_samples = 0, beg = 0;
    const uint32_t *depth = nullptr;     // host [rows], or NULL: to be counted
    const BvPtextToken *tokens = nullptr;  // host
    uint64_t n_tokens = 0;
    const uint8_t *h_text = nullptr, *d_text = nullptr;  // the tokens' text: an explicit tile's on the host, the pileup's on the device
    bool explicit_tile = false, host_planes = false;
};


// the planes the kernels read: PtextArgs' cell .. pitch and row0
struct PtextPlanes {
    const uint8_t *cell, *qual, *mapq;
    const uint16_t *rank;
    uint64_t pitch;
    uint32_t row0;
};

inline uint32_t ptext_tiles_of(uint32_t samples) { return (samples + BV_PTEXT_TILE - 1u) / BV_PTEXT_TILE; }

// The pileup's planes where they lie, or an explicit tile's rows of the call, packed at pitch P = up16(n_samples) with zeros behind
// the samples (`up`: the host's copy, alive until the stream is through)
int ptext_planes(bv_engine *e, BvPtextState *t, const bv_pileup_text *in, const TileView &v, hipStream_t st, std::vector<uint8_t> &up, PtextPlanes &a);

// The checks of a bv_pileup_text that bv_engine_pileup_text and bv_engine_pileup_text_parts share, and the tile it names
int ptext_check(bv_engine *e, const std::string &who, const bv_pileup_text *in, BvPileupView &pv, TileView &v);

}  // namespace bv_impl
