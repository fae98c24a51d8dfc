// bv_vcf.hip -- the per-sample GT:AB:SO:BP columns of VCF records expanded on the device (bv_engine_vcf_format,
// include/basevar_amd_vcf.h; the contract is INTEGRATION.md section 2h).  The bytes are defined at the head of bv_vcf_core.h,
// which a CPU harness compiles too; this file is their schedule.
//
// A line is its head (host text, uploaded -- or written in its place by bv_record_text.hip's kernel: bv_vcf_format_lines with
// BvVcfDeviceHeads) and one token of 4 or 17 bytes per sample.  Lines are cut into tiles of
// BV_VCF_TILE samples; one wave handles one (line, tile):
//   count  the tile's cell bytes, one 16-byte load a lane, -> covered cells of the tile
//   scan   one thread a line: the tile counts become the tiles' prefixes, their sum the line's covered count.  The line
//          lengths and line_off are then summed on the HOST: the call cannot size the text buffer before it knows the total,
//          so it waits for the counts in any case, and n_lines additions are nothing beside that wait.
//   write  64 samples a step: a 64-bit ballot of "covered" gives lane l its token's place, 4 l + 13 popc(mask below l) behind
//          the step's base, in an LDS image of the tile's output that is laid out as the text is modulo 16 and stored as one
//          piece (bv_text_image.h): neighbouring tiles and lines share 16-byte words, and every byte of the text has exactly
//          one writer.  Tile 0 copies the head, the last tile appends the '\n'.
// No atomics, no scratch, vector stores only.  Cells at pitch positions at or beyond n_samples are loaded with their 16-byte
// word and never looked at.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/basevar_amd_vcf.h"
#include "../../include/basevar_amd_diag.h"
#include "bv_chunk_stage.h"
#include "bv_device_text.h"
#include "bv_text_image.h"
#include "bv_vcf_core.h"

using namespace bv_impl;

namespace {

// Samples of a tile: one 16-byte load a lane.  The write kernel's LDS is the image (17 bytes a sample), the tile's two rows
// and the BP table, 21.5 KiB: seven workgroups fit a CU's 160 KiB.
constexpr uint32_t BV_VCF_TILE = 1024;
constexpr uint32_t kImageBytes = 16u + BV_VCF_TOK_CALL * BV_VCF_TILE + 16u;  // the text's offset modulo 16 in front, the '\n' behind
constexpr uint32_t kBpBytes = 256u * BV_VCF_BP_CHARS;
static_assert(BV_VCF_TILE == 64u * 16u, "a lane loads 16 cells of a tile");
static_assert(BV_VCF_CELL_NOCALL == BV_CELL_NOCALL && BV_VCF_CELL_REV == BV_CELL_REV, "bv_vcf_core.h restates the cell bits");

struct VcfArgs {
    const uint8_t *cell, *phred;  // [rows][pitch], 16-byte aligned rows
    uint64_t pitch;
    const uint32_t *row;          // [n_lines] row of line k
    const uint8_t *gt;            // [n_lines][4]
    const uint8_t *head;
    const uint64_t *head_off;     // [n_lines + 1]
    const uint64_t *line_off;     // [n_lines + 1] (write kernel)
    uint32_t *tile_cov;           // [n_lines][n_tiles]: covered cells of the tile; after the scan, of the tiles before it
    uint32_t *line_cov;           // [n_lines]
    const uint8_t *bp;            // [256][8]
    uint8_t *text;
    uint32_t n_lines, n_samples, n_tiles;
};

// where the tile's cells of line k begin in a plane
__device__ inline size_t tile_at(const VcfArgs &a, uint32_t k, uint32_t tile) { return (size_t)a.row[k] * a.pitch + (size_t)tile * BV_VCF_TILE; }

__global__ __launch_bounds__(64) void bv_vcf_count_kernel(VcfArgs a) {
    const auto [k, tile, cnt] = tile_of_block(a.n_tiles, a.n_samples, BV_VCF_TILE);
    const uint32_t lane = threadIdx.x;
    if (k >= a.n_lines) return;
    const uint4 c = tile_load16(a.cell + tile_at(a, k, tile), cnt, lane);
    const uint32_t valid = 16u * lane >= cnt ? 0u : min(16u, cnt - 16u * lane);  // the lane's bytes that are samples
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
    uint32_t n = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t v = valid > 4u * i ? min(4u, valid - 4u * i) : 0u;
        const uint32_t bytes = v == 4u ? 0xffffffffu : (1u << (8u * v)) - 1u;
        n += __popc(~w[i] & 0x08080808u & bytes);
    }
    n = wave_sum(n);
    if (lane == 0) a.tile_cov[(size_t)k * a.n_tiles + tile] = n;
}

__global__ __launch_bounds__(256) void bv_vcf_scan_kernel(VcfArgs a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.n_lines) return;
    uint32_t *tc = a.tile_cov + (size_t)k * a.n_tiles;
    uint32_t run = 0;
    for (uint32_t t = 0; t < a.n_tiles; ++t) {
        const uint32_t v = tc[t];
        tc[t] = run;
        run += v;
    }
    a.line_cov[k] = run;
}

__global__ __launch_bounds__(64) void bv_vcf_write_kernel(VcfArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t image[kImageBytes];
    __shared__ __attribute__((aligned(16))) uint8_t s_cell[BV_VCF_TILE];
    __shared__ __attribute__((aligned(16))) uint8_t s_phred[BV_VCF_TILE];
    __shared__ __attribute__((aligned(16))) uint8_t s_bp[kBpBytes];
    __shared__ uint8_t s_gt[4];
    const auto [k, tile, cnt] = tile_of_block(a.n_tiles, a.n_samples, BV_VCF_TILE);
    const uint32_t lane = threadIdx.x;
    if (k >= a.n_lines) return;
    const size_t at = tile_at(a, k, tile);
    reinterpret_cast<uint4 *>(s_cell)[lane] = tile_load16(a.cell + at, cnt, lane);
    reinterpret_cast<uint4 *>(s_phred)[lane] = tile_load16(a.phred + at, cnt, lane);
    for (uint32_t j = lane; j < kBpBytes / 16u; j += 64u) reinterpret_cast<uint4 *>(s_bp)[j] = reinterpret_cast<const uint4 *>(a.bp)[j];
    if (lane < 4u) s_gt[lane] = a.gt[4u * (size_t)k + lane];
    const uint64_t head_at = a.head_off[k], head_bytes = a.head_off[k + 1] - head_at, line_at = a.line_off[k];
    // where the tile's first token goes; the image starts at the 16-byte word of the text that holds it
    const uint64_t dst0 = line_at + head_bytes + (uint64_t)BV_VCF_TOK_NOCALL * tile * BV_VCF_TILE +
                          (uint64_t)(BV_VCF_TOK_CALL - BV_VCF_TOK_NOCALL) * a.tile_cov[(size_t)k * a.n_tiles + tile];
    const uint32_t shift = (uint32_t)(dst0 & 15u);
    __syncthreads();
    uint32_t base = shift;
    for (uint32_t s0 = 0; s0 < cnt; s0 += 64u) {
        const uint32_t s = s0 + lane;
        const bool active = s < cnt;
        const uint8_t c = active ? s_cell[s] : (uint8_t)BV_VCF_CELL_NOCALL;
        const uint64_t mask = __ballot(active && bv_vcf_covered(c));
        const uint32_t below = __popcll(mask & ((1ull << lane) - 1ull));
        if (active) bv_vcf_token(c, s_phred[s], s_gt, s_bp, image + base + BV_VCF_TOK_NOCALL * lane + (BV_VCF_TOK_CALL - BV_VCF_TOK_NOCALL) * below);
        base += BV_VCF_TOK_NOCALL * min(64u, cnt - s0) + (BV_VCF_TOK_CALL - BV_VCF_TOK_NOCALL) * (uint32_t)__popcll(mask);
    }
    if (tile + 1u == a.n_tiles) {
        if (lane == 0) image[base] = '\n';
        base += 1u;
    }
    if (tile == 0) head_copy(a.text + line_at, a.head + head_at, head_bytes, lane);
    // the tile's whole output is one piece of image [shift, base): the image has room for a tile, nothing was flushed on the way
    Piece p;
    piece_open(p, a.text, dst0, base - shift);
    p.fill = base;
    piece_flush(p, image, true, lane);
}

}  // namespace

// Per-engine state of bv_engine_vcf_format: the formatted text and what the kernels read beside the planes.
struct BvVcfState {
    DeviceText text;             // the formatted lines
    uint8_t *d_meta = nullptr;   // rows u32 [n], gt [n][4], head_off u64 [n + 1], the heads, line_off u64 [n + 1]
    uint8_t *d_cov = nullptr;    // tile_cov u32 [n][tiles], line_cov u32 [n]
    uint8_t *d_rows = nullptr;   // a host slab's named rows: cell [n][pitch], phred [n][pitch]
    uint8_t *d_bp = nullptr;     // BP [256][8]
    size_t meta_cap = 0, cov_cap = 0, rows_cap = 0;
};

void bv_vcf_state_free(BvVcfState *t) {
    if (!t) return;
    (void)hipSetDevice(t->text.device);
    for (uint8_t *b : {t->text.d_text, t->d_meta, t->d_cov, t->d_rows, t->d_bp})
        if (b) (void)hipFree(b);
    delete t;
}

namespace {

// What bv_engine_submit's check of a slab asks of the two planes that are read here
const char *check_planes(const bv_slab *s) {
    auto misaligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; };
    if (s->n_samples == 0 || s->pitch < s->n_samples || (s->pitch & 15ull)) return "pitch must be >= n_samples and a multiple of 16";
    if (!s->base_strand || !s->qual) return "base_strand and qual planes are required";
    if (misaligned(s->base_strand) || misaligned(s->qual)) return "planes must be 16-byte aligned";
    if (s->mem_kind != BV_MEM_HOST && s->mem_kind != BV_MEM_DEVICE) return "mem_kind must be BV_MEM_HOST or BV_MEM_DEVICE";
    if ((s->layout & ~BV_SLAB_RPR_TAGGED) || s->reserved_) return "unknown bv_slab.layout bits (built against another BV_ABI_VERSION?)";
    return nullptr;
}

// H: the heads and gt characters are not L's host bytes: H->fill queues the kernels that write them where the copy would
int vcf_format(bv_engine *e, BvVcfState *t, const bv_vcf_lines *L, const BvVcfDeviceHeads *H, const BvKeptRows &rows, bool host_rows, uint64_t *line_off, hipStream_t st) {
    const uint32_t n = L->n_lines, N = rows.n_samples;
    const uint32_t n_tiles = (N + BV_VCF_TILE - 1u) / BV_VCF_TILE;
    BV_HIP(e, hipSetDevice(t->text.device));
    if (!t->d_bp) {
        std::vector<uint8_t> bp(kBpBytes);
        if (!bv_vcf_bp_table(bp.data()))
            return fail(e, BV_ERR_HIP, "bv_engine_vcf_format: this host's \"%f\" of a BP value is not 8 characters: the lines cannot be laid out");
        uint8_t *d = nullptr;
        BV_HIP(e, hipMalloc(&d, kBpBytes));
        const hipError_t s = hipMemcpy(d, bp.data(), kBpBytes, hipMemcpyHostToDevice);
        if (s != hipSuccess) {
            (void)hipFree(d);
            return fail(e, BV_ERR_HIP, std::string("bv_engine_vcf_format: BP table: ") + hipGetErrorString(s));
        }
        t->d_bp = d;
    }
    // what the kernels read beside the planes, one upload: rows, gt, head_off, heads; line_off follows the counts
    const uint64_t *hoff = H ? H->head_off : L->head_off;
    const uint64_t head_lo = hoff[0], head_bytes = hoff[n] - head_lo;
    const size_t o_gt = up16(4ull * n), o_hoff = o_gt + up16(4ull * n), o_head = o_hoff + up16(8ull * (n + 1)), o_loff = o_head + up16(head_bytes),
                 meta = o_loff + up16(8ull * (n + 1));
    int rc = grow_device(e, &t->d_meta, &t->meta_cap, meta);
    if (rc == BV_OK) rc = grow_device(e, &t->d_cov, &t->cov_cap, 4ull * n * n_tiles + 4ull * n);
    if (rc != BV_OK) return rc;
    std::vector<uint8_t> h(o_loff, 0);
    uint32_t *h_row = reinterpret_cast<uint32_t *>(h.data());
    uint64_t *h_hoff = reinterpret_cast<uint64_t *>(h.data() + o_hoff);
    for (uint32_t k = 0; k < n; ++k) h_row[k] = host_rows ? k : L->site[k];
    if (!H) std::memcpy(h.data() + o_gt, L->gt, 4ull * n);
    for (uint32_t k = 0; k <= n; ++k) h_hoff[k] = hoff[k] - head_lo;
    if (!H && head_bytes) std::memcpy(h.data() + o_head, L->head + head_lo, head_bytes);
    BV_HIP(e, hipMemcpyAsync(t->d_meta, h.data(), o_loff, hipMemcpyHostToDevice, st));
    if (H) {
        rc = H->fill(H->ctx, t->d_meta + o_gt, t->d_meta + o_head, reinterpret_cast<const uint64_t *>(t->d_meta + o_hoff), st);
        if (rc != BV_OK) return rc;
    }
    VcfArgs a;
    a.cell = rows.cell; a.phred = rows.phred; a.pitch = rows.pitch;
    std::vector<uint8_t> up;
    if (host_rows) {  // the named rows of a host slab, the two planes only, packed in line order
        const size_t P = up16(N), plane = (size_t)n * P;
        rc = grow_device(e, &t->d_rows, &t->rows_cap, 2 * plane);
        if (rc != BV_OK) return rc;
        up.assign(2 * plane, BV_CELL_N);
        for (uint32_t k = 0; k < n; ++k) {
            std::memcpy(&up[(size_t)k * P], rows.cell + (size_t)L->site[k] * rows.pitch, N);
            std::memcpy(&up[plane + (size_t)k * P], rows.phred + (size_t)L->site[k] * rows.pitch, N);
        }
        BV_HIP(e, hipMemcpyAsync(t->d_rows, up.data(), 2 * plane, hipMemcpyHostToDevice, st));
        a.cell = t->d_rows; a.phred = t->d_rows + plane; a.pitch = P;
    }
    a.row = reinterpret_cast<const uint32_t *>(t->d_meta); a.gt = t->d_meta + o_gt;
    a.head_off = reinterpret_cast<const uint64_t *>(t->d_meta + o_hoff); a.head = t->d_meta + o_head;
    a.line_off = reinterpret_cast<const uint64_t *>(t->d_meta + o_loff);
    a.tile_cov = reinterpret_cast<uint32_t *>(t->d_cov); a.line_cov = a.tile_cov + (size_t)n * n_tiles;
    a.bp = t->d_bp; a.text = nullptr;
    a.n_lines = n; a.n_samples = N; a.n_tiles = n_tiles;
    hipLaunchKernelGGL(bv_vcf_count_kernel, dim3(n * n_tiles), dim3(64), 0, st, a);
    BV_HIP(e, hipGetLastError());
    hipLaunchKernelGGL(bv_vcf_scan_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, a);
    BV_HIP(e, hipGetLastError());
    std::vector<uint32_t> cov(n);
    BV_HIP(e, hipMemcpyAsync(cov.data(), a.line_cov, 4ull * n, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t k = 0; k < n; ++k) {
        if (cov[k] > N) return fail(e, BV_ERR_HIP, "bv_engine_vcf_format: line " + std::to_string(k) + " came back with more covered cells than samples");
        off[k + 1] = off[k] + bv_vcf_line_bytes(hoff[k + 1] - hoff[k], N, cov[k]);
    }
    rc = device_text_reserve(e, t->text, off[n]);
    if (rc != BV_OK) return rc;
    a.text = t->text.d_text;
    BV_HIP(e, hipMemcpyAsync(t->d_meta + o_loff, off.data(), 8ull * (n + 1), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bv_vcf_write_kernel, dim3(n * n_tiles), dim3(64), 0, st, a);
    BV_HIP(e, hipGetLastError());
    BV_HIP(e, hipStreamSynchronize(st));
    std::memcpy(line_off, off.data(), 8ull * (n + 1));
    device_text_done(t->text, off[n]);
    return BV_OK;
}

}  // namespace

extern "C" {

uint32_t bv_vcf_tile_samples(void) { return BV_VCF_TILE; }

}  // extern "C"

void bv_vcf_text_drop(bv_engine *e) {
    if (e->vcf) e->vcf->text.formatted = false;
}

int bv_vcf_format_lines(bv_engine *e, const char *who_, const bv_vcf_lines *L, const BvVcfDeviceHeads *H, uint64_t *line_off, void *stream_) {
    const std::string who = who_;
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    if (!L || !line_off) return fail(e, BV_ERR_INVALID_ARG, who + "null lines/line_off");
    if (L->reserved_) return fail(e, BV_ERR_INVALID_ARG, who + "reserved_ must be zero");
    const uint32_t n = L->n_lines;
    BvKeptRows rows;
    bool host_rows = false;
    if (n) {
        if (!L->site || (!H && (!L->head_off || !L->gt))) return fail(e, BV_ERR_INVALID_ARG, who + "null site/head_off/gt");
        for (uint32_t k = 0; !H && k < n; ++k)
            if (L->head_off[k + 1] < L->head_off[k]) return fail(e, BV_ERR_INVALID_ARG, who + "head_off out of order at line " + std::to_string(k));
        if (!H && !L->head && L->head_off[n] != L->head_off[0]) return fail(e, BV_ERR_INVALID_ARG, who + "null head");
        for (size_t i = 0; !H && i < 4ull * n; ++i)
            if (!bv_vcf_gt_char_ok(L->gt[i]))
                return fail(e, BV_ERR_INVALID_ARG, who + "gt of line " + std::to_string(i / 4) + ", base " + "ACGT"[i & 3] + " is none of '0', '.', '1' .. '4'");
        if (L->slab) {
            if (const char *why = check_planes(L->slab)) return fail(e, BV_ERR_INVALID_ARG, who + why);
            rows.cell = L->slab->base_strand; rows.phred = L->slab->qual; rows.pitch = L->slab->pitch;
            rows.n_rows = L->slab->n_sites; rows.n_samples = L->slab->n_samples;
            host_rows = L->slab->mem_kind == BV_MEM_HOST;
        } else if (!bv_text_kept_rows(e->text, &rows)) {
            return fail(e, BV_ERR_INVALID_ARG, who + "slab == NULL, and no bv_engine_text_submit has left rows on this engine");
        }
        for (uint32_t k = 0; k < n; ++k)
            if (L->site[k] >= rows.n_rows)
                return fail(e, BV_ERR_INVALID_ARG, who + "site " + std::to_string(L->site[k]) + " of line " + std::to_string(k) + " is beyond the " +
                                                       std::to_string(rows.n_rows) + (L->slab ? " rows of the slab" : " records of the last bv_engine_text_submit"));
        // one workgroup per (line, tile): a launch's grid has room for 2^26 of them
        if ((uint64_t)n * ((rows.n_samples + BV_VCF_TILE - 1u) / BV_VCF_TILE) >= (1ull << 26))
            return fail(e, BV_ERR_TOO_LARGE, who + "n_lines x tiles of a row exceeds 2^26: format fewer lines a call");
    }
    BvVcfState *t = text_state(e, e->vcf);
    t->text.formatted = false;  // deliberately here, not on entry as in bv_engine_pileup_text: a call whose arguments fail leaves the last text
    if (n == 0) return device_text_empty(t->text, line_off);
    return vcf_format(e, t, L, H, rows, host_rows, line_off, stream_ ? (hipStream_t)stream_ : e->stream);
}

extern "C" {

int bv_engine_vcf_format(bv_engine *e, const bv_vcf_lines *L, uint64_t *line_off, void *stream_) {
    return bv_vcf_format_lines(e, "bv_engine_vcf_format: ", L, nullptr, line_off, stream_);
}

int bv_engine_vcf_fetch(bv_engine *e, void *dst, uint64_t dst_capacity, int dst_mem_kind, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_vcf_fetch: null engine");
    return device_text_fetch(e, "bv_engine_vcf_fetch: ", "bv_engine_vcf_format", e->vcf ? &e->vcf->text : nullptr, dst, dst_capacity, dst_mem_kind, stream_);
}

int bv_engine_vcf_deflate(bv_engine *e, const uint64_t *block_off, uint32_t n_blocks, int level, uint8_t *dst, uint64_t dst_capacity,
                          uint64_t *member_off, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_vcf_deflate: null engine");
    return device_text_deflate(e, "bv_engine_vcf_deflate: ", "bv_engine_vcf_format", e->vcf ? &e->vcf->text : nullptr, block_off, n_blocks, level, dst, dst_capacity, member_off,
                               stream_);
}

}  // extern "C"
