// bv_deflate.hip -- text deflated into BGZF members on the device (bv_engine_bgzf_deflate, include/basevar_amd_bgzf.h; the
// contract is INTEGRATION.md section 2g).  The text goes to the device as bv_inflate.hip's members do: bv_chunk_stage.h.
//
// The host writer (host/bgzf_tabix.hpp) compresses every 0xff00-byte block of a `*.vcf.gz` / `*.cvg.gz` with one zlib
// deflate() on the one thread that keeps the output in order.  Here every block is one single-wave workgroup.  The encoder is
// bv_deflate_core.h, shared with a CPU harness: the block's text and the match table stay in LDS (63.8 KiB + 8 KiB of table +
// 0.6 KiB of chunk state + 4 KiB of CRC tables: two workgroups per CU), the lanes share the hashing, the match measuring, the
// table update and the CRC32, and walk the parse together.  What a block becomes depends on its text alone, so the device's
// members are the CPU build's, byte for byte.
//
// A member is first written to a slot of its own (its size is not known before), then the slots of a chunk are compacted on
// the device -- a prefix sum over the member sizes and a gather -- so that one contiguous run of members is copied back.
//
// BV_DEFLATE_SMALL (bv_engine_bgzf_deflate_level) is a second kernel over the same staging, scan and gather: the encoder of
// bv_deflate_small_core.h, dynamic Huffman codes over 16-, 8- and 4-byte grams (the same chunk matcher with three grams).
// Its three tables (24 KiB), the text and the Huffman workspace are 103 KiB of LDS: ONE workgroup per CU where the default
// level has two.  Its tokens wait in device memory between the parse and the coding (4 bytes per byte of text, allocated by
// the first call at that level).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/basevar_amd_bgzf.h"
#include "../../include/basevar_amd_diag.h"
#include "bv_deflate_core.h"
#include "bv_deflate_small_core.h"
#include "bv_chunk_stage.h"

using namespace bv_impl;

namespace {

constexpr uint32_t kSlotStride = 0x10020;  // bytes between two members' slots: 16-byte aligned, > 0xff00 + 31 + the 8 a word-wise reader may touch
constexpr uint32_t kChunkBlocks = 1024;    // blocks per staged chunk (two chunks in flight)
constexpr uint32_t kScanThreads = 256;
constexpr uint32_t kWinBytes = BV_DEF_MAX_BLOCK + BV_DEF_TEXT_PAD;  // a block's text in LDS
static_assert(BV_DEF_MAX_BLOCK + BV_DEF_MEMBER_EXTRA + 8u <= kSlotStride && kSlotStride % 16u == 0, "a member and a reader's last word fit a slot");

// one block of a staged chunk
struct BvDefBlock {
    uint64_t text_off;  // from the kernel's `text`
    uint32_t n;         // 1 .. BV_DEF_MAX_BLOCK
    uint32_t tok_at;    // BV_DEFLATE_SMALL: where the block's tokens wait, in units of 64 tokens; else 0
};

// the two aligned words around bytes [at, at + 4) of `base` (4-byte aligned), as one little-endian word
__device__ inline uint32_t word_at(const uint32_t *base, uint32_t at, bool second) {
    const uint32_t sh = 8u * (at & 3u);
    const uint32_t w0 = base[at >> 2];
    if (sh == 0) return w0;
    const uint32_t w1 = second ? base[(at >> 2) + 1u] : 0u;
    return (w0 >> sh) | (w1 << (32u - sh));
}

// the text of a block to the window, a word per lane and step.  Its place in memory has any alignment: a word of the window is
// cut from the two aligned words of global memory around it; the second is read only where it holds a byte of the block (an
// aligned word with one byte inside the buffer lies inside the buffer's pages).
__device__ inline void stage_text(const uint8_t *g, uint32_t n, uint8_t *win, uint32_t lane) {
    const uint32_t mis = (uint32_t)((uintptr_t)g & 3u);
    const uint32_t *ga = reinterpret_cast<const uint32_t *>(g - mis);
    uint32_t *w = reinterpret_cast<uint32_t *>(win);
    const uint32_t words = (n + 3u) / 4u;
    for (uint32_t j = lane; j < words; j += 64u) w[j] = word_at(ga, mis + 4u * j, 4u * j + 4u - mis < n);
    // (what lies behind the text in the window is read by bv_def_load4 and never used: cleared, so that no run differs)
    for (uint32_t j = words + lane; j < words + BV_DEF_TEXT_PAD / 4u && j < kWinBytes / 4u; j += 64u) w[j] = 0;
}

// What both levels' kernels begin with: block k of the launch, its text in `win` and the CRC tables in `crc_tab`.  False:
// there is nothing to code, and the whole workgroup leaves.
__device__ inline bool begin_block(const uint8_t *text, const BvDefBlock *meta, uint32_t nblk, uint32_t *sizes, uint8_t *win, uint32_t *crc_tab, BvDefBlock &m) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= nblk) return false;
    m = meta[k];
    if (m.n < 1u || m.n > BV_DEF_MAX_BLOCK) {  // (the host has refused such a block; nothing is read or written for it)
        if (lane == 0) sizes[k] = 0;
        return false;
    }
    bv_inf_crc_tables(crc_tab, lane, 64);
    stage_text(text + m.text_off, m.n, win, lane);
    __syncthreads();
    return true;
}

// the lanes' CRC shares combined: the xor over the wave
struct WaveXor {
    __device__ uint32_t operator()(uint32_t c) const {
        for (int d = 32; d > 0; d >>= 1) c ^= __shfl_xor(c, d, 64);
        return c;
    }
};

__global__ __launch_bounds__(64) void bv_bgzf_deflate_kernel(const uint8_t *__restrict__ text, const BvDefBlock *__restrict__ meta, uint32_t nblk,
                                                             uint8_t *__restrict__ slots, uint32_t *__restrict__ sizes) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kWinBytes];
    __shared__ BvDefState S;
    __shared__ uint32_t crc_tab[1024];
    BvDefBlock m;
    if (!begin_block(text, meta, nblk, sizes, win, crc_tab, m)) return;
    const uint32_t total = bv_def_member(win, m.n, slots + (size_t)blockIdx.x * kSlotStride, &S, crc_tab, threadIdx.x, 64, WaveXor());
    if (threadIdx.x == 0) sizes[blockIdx.x] = total;
}

// BV_DEFLATE_SMALL: one wave per block as above, with the encoder of bv_deflate_small_core.h.  tok: the chunk's token runs.
__global__ __launch_bounds__(64) void bv_bgzf_small_kernel(const uint8_t *__restrict__ text, const BvDefBlock *__restrict__ meta, uint32_t nblk,
                                                           uint8_t *__restrict__ slots, uint32_t *__restrict__ sizes, uint32_t *tok) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kWinBytes];
    __shared__ BvDefSmallState S;
    __shared__ uint32_t crc_tab[1024];
    BvDefBlock m;
    if (!begin_block(text, meta, nblk, sizes, win, crc_tab, m)) return;
    const uint32_t total = bv_def_small_member(win, m.n, slots + (size_t)blockIdx.x * kSlotStride, &S, tok + (size_t)m.tok_at * 64u, crc_tab, threadIdx.x, 64, WaveXor());
    if (threadIdx.x == 0) sizes[blockIdx.x] = total;
}

// bv_engine_deflate_code_lengths: one wave around bv_defs_code_lengths
__global__ __launch_bounds__(64) void bv_deflate_code_lengths_kernel(const uint32_t *__restrict__ counts, uint32_t nsym, uint32_t limit, uint8_t *__restrict__ lengths,
                                                                     uint32_t *__restrict__ rounds) {
    __shared__ BvDefsHuff H;
    __shared__ uint32_t cnt[BV_DEFS_MAX_SYMS];
    __shared__ uint8_t len[BV_DEFS_MAX_SYMS];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < nsym; i += 64u) cnt[i] = counts[i];
    __syncthreads();
    const uint32_t r = bv_defs_code_lengths(cnt, nsym, limit, len, &H, lane, 64);
    for (uint32_t i = lane; i < nsym; i += 64u) lengths[i] = len[i];
    if (lane == 0) *rounds = r;
}

// off[0] = 0, off[k + 1] = off[k] + sizes[k]: one workgroup, every thread a contiguous share
__global__ __launch_bounds__(kScanThreads) void bv_bgzf_deflate_scan_kernel(const uint32_t *__restrict__ sizes, uint32_t nblk, uint32_t *__restrict__ off) {
    __shared__ uint32_t part[kScanThreads];
    const uint32_t t = threadIdx.x, per = (nblk + kScanThreads - 1u) / kScanThreads;
    const uint32_t lo = t * per < nblk ? t * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    uint32_t sum = 0;
    for (uint32_t k = lo; k < hi; ++k) sum += sizes[k];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < kScanThreads; ++i) { const uint32_t v = part[i]; part[i] = run; run += v; }
        off[0] = 0;
    }
    __syncthreads();
    uint32_t run = part[t];
    for (uint32_t k = lo; k < hi; ++k) { run += sizes[k]; off[k + 1u] = run; }
}

// member k from its slot to packed + off[k]: bytes up to the first aligned word of the destination, whole words (cut from the
// slot's aligned words; a slot has room behind the longest member for the last of them), bytes behind them
__global__ __launch_bounds__(256) void bv_bgzf_deflate_gather_kernel(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ off, uint32_t nblk,
                                                                    uint8_t *__restrict__ packed) {
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    if (k >= nblk) return;
    const uint32_t size = off[k + 1u] - off[k];
    const uint8_t *src = slots + (size_t)k * kSlotStride;
    uint8_t *dst = packed + off[k];
    const uint32_t align = (uint32_t)(-(uintptr_t)dst & 3u), head = align < size ? align : size;
    const uint32_t words = (size - head) / 4u, tail = head + words * 4u;
    if (t < head) dst[t] = src[t];
    const uint32_t *sa = reinterpret_cast<const uint32_t *>(src);
    uint32_t *da = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t j = t; j < words; j += 256u) da[j] = word_at(sa, head + 4u * j, true);
    if (tail + t < size) dst[tail + t] = src[tail + t];
}

}  // namespace

// Per-engine staging of bv_engine_bgzf_deflate: the chunks of text (host text only), each with its block table behind it, and
// the running sums that come back (bv_chunk_stage.h has the rule of their reuse); per slot the member slots, the packed
// members, the member sizes and their running sums on the device.
struct BvDeflateState {
    int device = 0;
    ChunkStage in;
    // Touched on the call's stream alone, by the slot's kernels and the copies behind them.  The copy back of `d_packed` is
    // queued by finish(), which bgzf_deflate calls for chunk k before it issues chunk k + 2: stream order keeps them apart.
    struct Slot {
        uint8_t *d_slots = nullptr, *d_packed = nullptr;
        uint32_t *d_sums = nullptr;  // sizes [kChunkBlocks], then off [kChunkBlocks + 1]
        uint32_t *d_tok = nullptr;   // BV_DEFLATE_SMALL: the blocks' tokens between parse and coding (never allocated at the default level)
        size_t slots_cap = 0, packed_cap = 0, sums_cap = 0, tok_cap = 0;
    } slot[2];
    bool lds_ok = false, lds_ok_small = false;  // the kernel's LDS was accepted
    uint8_t *d_diag = nullptr;  // bv_engine_deflate_code_lengths: counts, lengths, rounds
};

void bv_deflate_state_free(BvDeflateState *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    chunk_stage_free(t->in);
    for (BvDeflateState::Slot &sl : t->slot)
        for (void *b : {(void *)sl.d_slots, (void *)sl.d_packed, (void *)sl.d_sums, (void *)sl.d_tok})
            if (b) (void)hipFree(b);
    if (t->d_diag) (void)hipFree(t->d_diag);
    delete t;
}

namespace {

struct Chunk {
    uint32_t first, count;
    uint64_t text_lo, text_bytes;  // the text its blocks span (block_off[first] .. block_off[first + count])
};

int bgzf_deflate(bv_engine *e, BvDeflateState *t, const uint8_t *text, bool host_text, const uint64_t *block_off, uint32_t n, int level, uint8_t *dst,
                 uint64_t *member_off, hipStream_t st) {
    BV_HIP(e, hipSetDevice(t->device));
    int rc = chunk_stage_begin(e, t->in, st);
    if (rc == BV_OK && level == BV_DEFLATE_SMALL)
        rc = kernel_lds_fits(e, "bv_engine_bgzf_deflate_level: the small level's kernel", reinterpret_cast<const void *>(bv_bgzf_small_kernel), t->device, &t->lds_ok_small);
    else if (rc == BV_OK)
        rc = kernel_lds_fits(e, "bv_engine_bgzf_deflate: the deflate kernel", reinterpret_cast<const void *>(bv_bgzf_deflate_kernel), t->device, &t->lds_ok);
    if (rc != BV_OK) return rc;
    const uint32_t per = (uint32_t)chunk_limit_from_env("BASEVAR_AMD_DEFLATE_CHUNK_BLOCKS", kChunkBlocks);
    std::vector<Chunk> chunks;
    size_t in_max = 0, tok_max = 0;
    for (uint32_t k = 0; k < n; k += per) {
        const uint32_t count = std::min(per, n - k);
        chunks.push_back(Chunk{k, count, block_off[k], block_off[k + count] - block_off[k]});
        in_max = std::max<size_t>(in_max, chunks.back().text_bytes);
        if (level != BV_DEFLATE_SMALL) continue;
        size_t room = 0;
        for (uint32_t j = k; j < k + count; ++j) room += BV_DEFS_TOK_ROOM((uint32_t)(block_off[j + 1] - block_off[j]));
        tok_max = std::max(tok_max, room);
    }
    const size_t blocks_max = std::min<size_t>(per, n);
    // a staged chunk: the text (host text only; the kernel reads whole words around it), then the block table
    rc = chunk_stage_reserve(e, t->in, (host_text ? up16(in_max + 4) : 0) + sizeof(BvDefBlock) * blocks_max, sizeof(uint32_t) * (kChunkBlocks + 1));
    if (rc != BV_OK) return rc;
    for (BvDeflateState::Slot &sl : t->slot) {
        if ((rc = grow_device(e, &sl.d_slots, &sl.slots_cap, blocks_max * kSlotStride)) != BV_OK) return rc;
        if ((rc = grow_device(e, &sl.d_packed, &sl.packed_cap, in_max + (size_t)BV_DEF_MEMBER_EXTRA * blocks_max)) != BV_OK) return rc;
        if ((rc = grow_device(e, &sl.d_sums, &sl.sums_cap, sizeof(uint32_t) * (2 * kChunkBlocks + 1))) != BV_OK) return rc;
        if (level == BV_DEFLATE_SMALL && (rc = grow_device(e, &sl.d_tok, &sl.tok_cap, sizeof(uint32_t) * tok_max)) != BV_OK) return rc;
    }
    // a chunk's packed members are copied back while the next chunk is being coded: `finish` is one chunk behind `issue`
    auto finish = [&](size_t ci) -> int {
        const Chunk &c = chunks[ci];
        const unsigned s = ci & 1u;
        const int rw = chunk_stage_wait_done(e, t->in, s);  // the slot's kernels and the copy of its running sums are through
        if (rw != BV_OK) return rw;
        const uint32_t *off = reinterpret_cast<const uint32_t *>(t->in.slot[s].back);
        for (uint32_t j = 0; j < c.count; ++j) {
            const uint32_t size = off[j + 1] - off[j];
            if (size < BV_INF_MIN_MEMBER || size > block_off[c.first + j + 1] - block_off[c.first + j] + BV_DEF_MEMBER_EXTRA)
                return fail(e, BV_ERR_HIP, "bv_engine_bgzf_deflate: block " + std::to_string(c.first + j) + " came back as a member of " +
                                               std::to_string(size) + " bytes");
            member_off[c.first + j + 1] = member_off[c.first + j] + size;
        }
        BV_HIP(e, hipMemcpyAsync(dst + member_off[c.first], t->slot[s].d_packed, off[c.count], hipMemcpyDeviceToHost, st));
        return BV_OK;
    };
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const Chunk &c = chunks[ci];
        const unsigned s = ci & 1u;
        // (finish(ci - 2) has waited for the slot's kernels on the host: the stricter wait, kept because it reads the sums)
        if ((rc = chunk_stage_fill(e, t->in, s)) != BV_OK) return rc;
        uint8_t *h_in = t->in.slot[s].h;
        const size_t meta_at = host_text ? up16(c.text_bytes + 4) : 0;
        if (host_text) std::memcpy(h_in, text + c.text_lo, c.text_bytes);
        BvDefBlock *h_meta = reinterpret_cast<BvDefBlock *>(h_in + meta_at);
        size_t tok_at = 0;
        for (uint32_t j = 0; j < c.count; ++j) {
            BvDefBlock &m = h_meta[j];
            const uint64_t a = block_off[c.first + j];
            m.text_off = host_text ? a - c.text_lo : a;
            m.n = (uint32_t)(block_off[c.first + j + 1] - a);
            m.tok_at = 0;
            if (level == BV_DEFLATE_SMALL) {
                m.tok_at = (uint32_t)(tok_at / 64u);
                tok_at += BV_DEFS_TOK_ROOM(m.n);
            }
        }
        if ((rc = chunk_stage_upload(e, t->in, s, meta_at + sizeof(BvDefBlock) * c.count, st)) != BV_OK) return rc;
        const uint8_t *d_in = t->in.slot[s].d;
        const BvDeflateState::Slot &sl = t->slot[s];
        uint32_t *d_sizes = sl.d_sums, *d_off = sl.d_sums + kChunkBlocks;
        if (level == BV_DEFLATE_SMALL)
            hipLaunchKernelGGL(bv_bgzf_small_kernel, dim3(c.count), dim3(64), 0, st, host_text ? d_in : text,
                               reinterpret_cast<const BvDefBlock *>(d_in + meta_at), c.count, sl.d_slots, d_sizes, sl.d_tok);
        else
            hipLaunchKernelGGL(bv_bgzf_deflate_kernel, dim3(c.count), dim3(64), 0, st, host_text ? d_in : text,
                               reinterpret_cast<const BvDefBlock *>(d_in + meta_at), c.count, sl.d_slots, d_sizes);
        BV_HIP(e, hipGetLastError());
        hipLaunchKernelGGL(bv_bgzf_deflate_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t *)d_sizes, c.count, d_off);
        BV_HIP(e, hipGetLastError());
        hipLaunchKernelGGL(bv_bgzf_deflate_gather_kernel, dim3(c.count), dim3(256), 0, st, (const uint8_t *)sl.d_slots, (const uint32_t *)d_off, c.count,
                           sl.d_packed);
        BV_HIP(e, hipGetLastError());
        BV_HIP(e, hipMemcpyAsync(t->in.slot[s].back, d_off, sizeof(uint32_t) * (c.count + 1), hipMemcpyDeviceToHost, st));
        if ((rc = chunk_stage_done(e, t->in, s, st)) != BV_OK) return rc;
        if (ci >= 1 && (rc = finish(ci - 1)) != BV_OK) return rc;
    }
    if ((rc = finish(chunks.size() - 1)) != BV_OK) return rc;
    BV_HIP(e, hipStreamSynchronize(st));
    return BV_OK;
}

}  // namespace

extern "C" {

int bv_engine_bgzf_deflate_level(bv_engine *e, const void *text, uint64_t text_bytes, int text_mem_kind, const uint64_t *block_off, uint32_t n_blocks,
                                 int level, uint8_t *dst, uint64_t dst_capacity, uint64_t *member_off, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_bgzf_deflate: null engine");
    if (level != BV_DEFLATE_FAST && level != BV_DEFLATE_SMALL)
        return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_deflate_level: level must be BV_DEFLATE_FAST or BV_DEFLATE_SMALL");
    if (!member_off) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_deflate: null member_off");
    if (text_mem_kind != BV_MEM_HOST && text_mem_kind != BV_MEM_DEVICE)
        return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_deflate: text_mem_kind must be BV_MEM_HOST or BV_MEM_DEVICE");
    member_off[0] = 0;
    if (n_blocks == 0) return BV_OK;
    if (!text || !block_off || !dst) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_deflate: null text/block_off/dst");
    for (uint32_t k = 0; k < n_blocks; ++k) {
        const uint64_t a = block_off[k], b = block_off[k + 1];
        if (b < a || b > text_bytes)
            return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_deflate: block " + std::to_string(k) + ": block_off out of order or beyond text_bytes");
        if (b - a < 1 || b - a > BV_DEF_MAX_BLOCK)
            return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_deflate: block " + std::to_string(k) + " is " + std::to_string(b - a) +
                                                             " bytes: a BGZF block has 1 to 65280");
    }
    const uint64_t need = text_bytes + (uint64_t)BV_DEF_MEMBER_EXTRA * n_blocks;
    if (dst_capacity < need)
        return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_deflate: dst_capacity " + std::to_string(dst_capacity) + " < text_bytes + 31 * n_blocks = " +
                                                         std::to_string(need));
    return bgzf_deflate(e, engine_state(e, e->deflate), static_cast<const uint8_t *>(text), text_mem_kind == BV_MEM_HOST, block_off, n_blocks, level, dst,
                        member_off,
                        stream_ ? (hipStream_t)stream_ : e->stream);
}

int bv_engine_bgzf_deflate(bv_engine *e, const void *text, uint64_t text_bytes, int text_mem_kind, const uint64_t *block_off, uint32_t n_blocks,
                           uint8_t *dst, uint64_t dst_capacity, uint64_t *member_off, void *stream_) {
    return bv_engine_bgzf_deflate_level(e, text, text_bytes, text_mem_kind, block_off, n_blocks, BV_DEFLATE_FAST, dst, dst_capacity, member_off, stream_);
}

int bv_engine_deflate_code_lengths(bv_engine *e, const uint32_t *counts, uint32_t n_symbols, uint32_t limit, uint8_t *lengths_out, uint32_t *rounds_out,
                                   void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_deflate_code_lengths: null engine");
    if (!counts || !lengths_out || !rounds_out) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_deflate_code_lengths: null counts/lengths_out/rounds_out");
    if (n_symbols < 2 || n_symbols > BV_DEFS_MAX_SYMS || limit < 1 || limit > 15 || n_symbols > (1u << limit))
        return fail(e, BV_ERR_INVALID_ARG, "bv_engine_deflate_code_lengths: 2 to 286 symbols, a limit of 1 to 15 bits, and no more symbols than 2^limit");
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n_symbols; ++i) sum += counts[i];
    if (sum >> 32) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_deflate_code_lengths: the counts add up to 2^32 or more");
    BvDeflateState *t = engine_state(e, e->deflate);
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    BV_HIP(e, hipSetDevice(t->device));
    constexpr size_t kLenAt = sizeof(uint32_t) * BV_DEFS_MAX_SYMS, kRoundsAt = kLenAt + 288;
    if (!t->d_diag) BV_HIP(e, hipMalloc(&t->d_diag, kRoundsAt + sizeof(uint32_t)));
    BV_HIP(e, hipMemcpyAsync(t->d_diag, counts, sizeof(uint32_t) * n_symbols, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bv_deflate_code_lengths_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(t->d_diag), n_symbols, limit, t->d_diag + kLenAt,
                       reinterpret_cast<uint32_t *>(t->d_diag + kRoundsAt));
    BV_HIP(e, hipGetLastError());
    BV_HIP(e, hipMemcpyAsync(lengths_out, t->d_diag + kLenAt, n_symbols, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipMemcpyAsync(rounds_out, t->d_diag + kRoundsAt, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    return BV_OK;
}

}  // extern "C"
