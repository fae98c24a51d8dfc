// bv_inflate.hip -- BGZF members inflated on the device (bv_engine_bgzf_inflate, include/basevar_amd_bgzf.h; the contract is
// INTEGRATION.md section 2f).
//
// A BGZF file is a chain of independent DEFLATE members of at most 64 KiB of text each; the reference inflates them one after
// the other with zlib on the host (htslib's bgzf reader behind src/basetype_caller.cpp:428).  Here every member is one
// single-wave workgroup.  The decoder itself is bv_inflate_core.h, shared with a CPU harness that holds it to zlib under
// ASan + UBSan: all 64 lanes walk the Huffman symbols with the same values (no divergence, table reads are LDS broadcasts) and
// share what is wide -- the fill of the decode tables, the bytes of a match or a stored block, the CRC32 and the write-out.
// The member's whole output window stays in LDS (64 KiB + 7.5 KiB of tables + 4 KiB of CRC tables: two workgroups per CU), so
// a match reads what the wave wrote a few instructions earlier at LDS latency, and the text leaves the kernel once, 16 bytes
// per lane.  A member that is damaged ends with a status byte; its bounds are the core's (payload length, ISIZE, bytes
// written), none of them taken from the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/basevar_amd_bgzf.h"
#include "bv_inflate_core.h"
#include "bv_engine_impl.h"

using namespace bv_impl;

static_assert(BV_INF_OK == BV_BGZF_OK && BV_INF_BAD_HEADER == BV_BGZF_BAD_HEADER && BV_INF_BAD_DEFLATE == BV_BGZF_BAD_DEFLATE &&
                  BV_INF_BAD_SIZE == BV_BGZF_BAD_SIZE && BV_INF_BAD_CRC == BV_BGZF_BAD_CRC,
              "bv_inflate_core.h and basevar_amd_bgzf.h name the member statuses differently");

namespace {

// one member of a staged chunk
struct BvInfMember {
    uint64_t out_off;  // where its text goes, from the kernel's `out`
    uint32_t in_off;   // its DEFLATE payload inside the chunk
    uint32_t in_len;
    uint32_t isize, crc;
    uint32_t pre;      // the status the header left it with; the payload is looked at only when it is BV_BGZF_OK
    uint32_t reserved_;
};

__global__ __launch_bounds__(64) void bv_bgzf_inflate_kernel(const uint8_t *__restrict__ in, const BvInfMember *__restrict__ meta, uint32_t n,
                                                             uint8_t *__restrict__ out, uint8_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t win[BV_INF_MAX_ISIZE];
    __shared__ BvInfTables T;
    __shared__ uint32_t crc_tab[1024];
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= n) return;
    const BvInfMember m = meta[k];
    int st = (int)m.pre;
    if (st == BV_INF_OK && m.isize > BV_INF_MAX_ISIZE) st = BV_INF_BAD_SIZE;
    if (st == BV_INF_OK) {
        bv_inf_crc_tables(crc_tab, lane, 64);
        st = bv_inf_stream(in + m.in_off, m.in_len, win, m.isize, &T, lane, 64);
        __syncthreads();
    }
    if (st == BV_INF_OK) {
        uint32_t c = bv_inf_crc_share(win, m.isize, lane, crc_tab);
        for (int d = 32; d > 0; d >>= 1) c ^= __shfl_xor(c, d, 64);
        if (~c != m.crc) st = BV_INF_BAD_CRC;
    }
    if (st == BV_INF_OK) {
        // the window to its place in `out`: single bytes up to the first 16-byte line, whole lines, single bytes behind them
        uint8_t *g = out + m.out_off;
        const uint32_t align = (uint32_t)(-(uintptr_t)g & 15u), head = align < m.isize ? align : m.isize;
        const uint32_t lines = (m.isize - head) / 16u, tail = head + lines * 16u;
        if (lane < head) g[lane] = win[lane];
        for (uint32_t v = lane; v < lines; v += 64u) {
            const uint8_t *w = win + head + v * 16u;
            uint32_t x[4];
            for (int q = 0; q < 4; ++q)
                x[q] = w[4 * q] | ((uint32_t)w[4 * q + 1] << 8) | ((uint32_t)w[4 * q + 2] << 16) | ((uint32_t)w[4 * q + 3] << 24);
            *reinterpret_cast<uint4 *>(g + head + v * 16u) = make_uint4(x[0], x[1], x[2], x[3]);
        }
        if (tail + lane < m.isize) g[tail + lane] = win[tail + lane];
    }
    if (lane == 0) status[k] = (uint8_t)st;
}

constexpr size_t kInChunkBytes = (size_t)32 << 20;  // compressed bytes per staged chunk (two chunks in flight)
constexpr size_t kOutPerIn = 4;                     // inflated bytes a chunk may hold, per compressed byte of its capacity
constexpr uint32_t kChunkMembers = 16384;

}  // namespace

// Per-engine staging of bv_engine_bgzf_inflate: two pinned host + two device chunks of compressed bytes and member tables, and
// (for a host destination) two device chunks of inflated text.
struct BvBgzfState {
    int device = 0;
    hipStream_t cs = nullptr;  // copy stream of the compressed chunks
    hipEvent_t ev_copied[2] = {}, ev_done[2] = {};
    uint8_t *h_in[2] = {}, *d_in[2] = {};
    size_t in_cap = 0;
    BvInfMember *h_meta[2] = {}, *d_meta[2] = {};
    uint8_t *d_out[2] = {};
    size_t out_cap = 0;
    uint8_t *d_status = nullptr;
    size_t status_cap = 0;
    bool ready = false;  // the kernel's LDS was accepted and the stream, events and member tables exist
};

void bv_bgzf_state_free(BvBgzfState *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->cs) (void)hipStreamSynchronize(t->cs);
    for (int k = 0; k < 2; ++k) {
        if (t->h_in[k]) (void)hipHostFree(t->h_in[k]);
        if (t->d_in[k]) (void)hipFree(t->d_in[k]);
        if (t->h_meta[k]) (void)hipHostFree(t->h_meta[k]);
        if (t->d_meta[k]) (void)hipFree(t->d_meta[k]);
        if (t->d_out[k]) (void)hipFree(t->d_out[k]);
        if (t->ev_copied[k]) (void)hipEventDestroy(t->ev_copied[k]);
        if (t->ev_done[k]) (void)hipEventDestroy(t->ev_done[k]);
    }
    if (t->d_status) (void)hipFree(t->d_status);
    if (t->cs) (void)hipStreamDestroy(t->cs);
    delete t;
}

namespace {

int ensure_staging(bv_engine *e, BvBgzfState *t, size_t in_bytes, size_t out_bytes, size_t n_members) {
    if (!t->ready) {
        // the kernel's LDS (window + tables) is more than the 64 KiB every launch may have: ask once whether this device takes it
        hipFuncAttributes fa;
        BV_HIP(e, hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(bv_bgzf_inflate_kernel)));
        int lds_max = 0;
        BV_HIP(e, hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, t->device));
        if (fa.sharedSizeBytes > (size_t)lds_max)
            return fail(e, BV_ERR_NO_DEVICE, "bv_engine_bgzf_inflate: the inflate kernel needs " + std::to_string(fa.sharedSizeBytes) +
                                                           " bytes of LDS per workgroup, the device offers " + std::to_string(lds_max));
        if (!t->cs) BV_HIP(e, hipStreamCreateWithFlags(&t->cs, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {  // (each object if it is missing: a call that failed half-way is taken up where it stopped)
            if (!t->ev_copied[k]) BV_HIP(e, hipEventCreateWithFlags(&t->ev_copied[k], hipEventDisableTiming));
            if (!t->ev_done[k]) BV_HIP(e, hipEventCreateWithFlags(&t->ev_done[k], hipEventDisableTiming));
            if (!t->h_meta[k]) BV_HIP(e, hipHostMalloc(reinterpret_cast<void **>(&t->h_meta[k]), sizeof(BvInfMember) * kChunkMembers));
            if (!t->d_meta[k]) BV_HIP(e, hipMalloc(reinterpret_cast<void **>(&t->d_meta[k]), sizeof(BvInfMember) * kChunkMembers));
        }
        t->ready = true;
    }
    if (in_bytes > t->in_cap) {
        for (int k = 0; k < 2; ++k) {
            if (t->h_in[k]) BV_HIP(e, hipHostFree(t->h_in[k]));
            if (t->d_in[k]) BV_HIP(e, hipFree(t->d_in[k]));
            t->h_in[k] = t->d_in[k] = nullptr;
        }
        t->in_cap = 0;
        for (int k = 0; k < 2; ++k) {
            BV_HIP(e, hipHostMalloc(reinterpret_cast<void **>(&t->h_in[k]), in_bytes));
            BV_HIP(e, hipMalloc(reinterpret_cast<void **>(&t->d_in[k]), in_bytes));
        }
        t->in_cap = in_bytes;
    }
    if (out_bytes > t->out_cap) {
        for (int k = 0; k < 2; ++k) {
            if (t->d_out[k]) BV_HIP(e, hipFree(t->d_out[k]));
            t->d_out[k] = nullptr;
        }
        t->out_cap = 0;
        for (int k = 0; k < 2; ++k) BV_HIP(e, hipMalloc(reinterpret_cast<void **>(&t->d_out[k]), out_bytes));
        t->out_cap = out_bytes;
    }
    return grow_device(e, &t->d_status, &t->status_cap, n_members);
}

struct Chunk {
    uint32_t first, count;
    size_t in_bytes, out_bytes;
};

int bgzf_inflate(bv_engine *e, BvBgzfState *t, const bv_bgzf_members *mb, const std::vector<BvBgzfMember> &hd, const std::vector<uint8_t> &pre,
                 uint8_t *dst, bool host_dst, const uint64_t *out_pos, uint8_t *status, hipStream_t st) {
    const uint32_t n = mb->n_members;
    BV_HIP(e, hipSetDevice(t->device));
    // a call that failed part-way may have left work queued: the staging is free only once it is through
    if (t->cs) BV_HIP(e, hipStreamSynchronize(t->cs));
    BV_HIP(e, hipStreamSynchronize(st));
    // (BASEVAR_AMD_TEXT_CHUNK_BYTES: a smaller chunk, for tests of the staging's reuse; never above the default)
    size_t in_cap = kInChunkBytes;
    if (const char *v = std::getenv("BASEVAR_AMD_TEXT_CHUNK_BYTES")) {
        const unsigned long long x = std::strtoull(v, nullptr, 10);
        if (x > 0 && x < kInChunkBytes) in_cap = (size_t)x;
    }
    in_cap = std::max<size_t>(in_cap, 65536);  // one member always fits
    const size_t out_cap = in_cap * kOutPerIn;
    std::vector<Chunk> chunks;
    size_t in_max = 0, out_max = 0;
    for (uint32_t k = 0; k < n;) {
        Chunk c{k, 0, 0, 0};
        while (k < n && c.count < kChunkMembers) {
            const size_t len = mb->member_off[k + 1] - mb->member_off[k], text = hd[k].isize;
            if (c.count && (c.in_bytes + len > in_cap || c.out_bytes + text > out_cap)) break;
            c.in_bytes += len; c.out_bytes += text;
            ++c.count; ++k;
        }
        in_max = std::max(in_max, c.in_bytes); out_max = std::max(out_max, c.out_bytes);
        chunks.push_back(c);
    }
    int rc = ensure_staging(e, t, in_max, host_dst ? std::max<size_t>(out_max, 16) : 0, n);
    if (rc != BV_OK) return rc;
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const Chunk &c = chunks[ci];
        const unsigned s = ci & 1u;
        if (ci >= 2) BV_HIP(e, hipEventSynchronize(t->ev_done[s]));  // the slot's kernel (and its copy back) is through
        size_t at = 0;
        for (uint32_t j = 0; j < c.count; ++j) {
            const uint32_t k = c.first + j;
            const size_t len = mb->member_off[k + 1] - mb->member_off[k];
            std::memcpy(t->h_in[s] + at, mb->data + mb->member_off[k], len);
            BvInfMember &m = t->h_meta[s][j];
            m.out_off = host_dst ? out_pos[k] - out_pos[c.first] : out_pos[k];
            m.in_off = (uint32_t)(at + hd[k].payload_off); m.in_len = hd[k].payload_len;
            m.isize = hd[k].isize; m.crc = hd[k].crc; m.pre = pre[k]; m.reserved_ = 0;
            at += len;
        }
        BV_HIP(e, hipMemcpyAsync(t->d_in[s], t->h_in[s], c.in_bytes, hipMemcpyHostToDevice, t->cs));
        BV_HIP(e, hipMemcpyAsync(t->d_meta[s], t->h_meta[s], sizeof(BvInfMember) * c.count, hipMemcpyHostToDevice, t->cs));
        BV_HIP(e, hipEventRecord(t->ev_copied[s], t->cs));
        BV_HIP(e, hipStreamWaitEvent(st, t->ev_copied[s], 0));
        hipLaunchKernelGGL(bv_bgzf_inflate_kernel, dim3(c.count), dim3(64), 0, st, (const uint8_t *)t->d_in[s], (const BvInfMember *)t->d_meta[s],
                           c.count, host_dst ? t->d_out[s] : dst, t->d_status + c.first);
        BV_HIP(e, hipGetLastError());
        if (host_dst && c.out_bytes)
            BV_HIP(e, hipMemcpyAsync(dst + out_pos[c.first], t->d_out[s], c.out_bytes, hipMemcpyDeviceToHost, st));
        BV_HIP(e, hipEventRecord(t->ev_done[s], st));
    }
    BV_HIP(e, hipMemcpyAsync(status, t->d_status, n, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    return BV_OK;
}

BvBgzfState *state_of(bv_engine *e) {
    if (!e->bgzf) {
        e->bgzf = new BvBgzfState();
        e->bgzf->device = e->cfg.device;
    }
    return e->bgzf;
}

}  // namespace

// The wrappers of the members, on the host: ISIZE is what places every member's text, so it is needed before anything is
// launched.  hd[k].isize is 0 for a member that pre[k] already refuses (a bad header, an ISIZE no BGZF member has).
int bv_bgzf_headers(bv_engine *e, const char *who, const bv_bgzf_members *mb, std::vector<BvBgzfMember> &hd, std::vector<uint8_t> &pre) {
    const uint32_t n = mb->n_members;
    for (uint32_t k = 0; k < n; ++k) {
        const uint64_t a = mb->member_off[k], b = mb->member_off[k + 1];
        if (b < a || b > mb->data_bytes)
            return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": member " + std::to_string(k) + ": member_off out of order or beyond data_bytes");
        if (b - a < BV_INF_MIN_MEMBER || b - a > 65536u)
            return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": member " + std::to_string(k) + " is " + std::to_string(b - a) +
                                                             " bytes: a BGZF member has 26 to 65536");
    }
    hd.resize(n);
    pre.resize(n);
    for (uint32_t k = 0; k < n; ++k) {
        int s = bv_bgzf_member_parse(mb->data + mb->member_off[k], mb->member_off[k + 1] - mb->member_off[k], &hd[k]);
        if (s == BV_INF_OK && hd[k].isize > BV_INF_MAX_ISIZE) s = BV_INF_BAD_SIZE;
        if (s != BV_INF_OK) hd[k].isize = 0;
        pre[k] = (uint8_t)s;
    }
    return BV_OK;
}

// Member k's text to d_dst + out_pos[k] (device memory of the engine's device); status[n_members] on the host.  Blocks.
int bv_bgzf_inflate_placed(bv_engine *e, const bv_bgzf_members *mb, const std::vector<BvBgzfMember> &hd, const std::vector<uint8_t> &pre,
                           const uint64_t *out_pos, uint8_t *d_dst, uint8_t *status, hipStream_t st) {
    return bgzf_inflate(e, state_of(e), mb, hd, pre, d_dst, false, out_pos, status, st);
}

extern "C" {

int bv_engine_bgzf_inflate(bv_engine *e, const bv_bgzf_members *mb, void *dst, uint64_t dst_capacity, int mem_kind, uint64_t *dst_off,
                           uint8_t *status, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_bgzf_inflate: null engine");
    if (!mb || !dst_off) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_inflate: null members/dst_off");
    if (mb->reserved_) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_inflate: reserved_ must be zero");
    if (mem_kind != BV_MEM_HOST && mem_kind != BV_MEM_DEVICE)
        return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_inflate: mem_kind must be BV_MEM_HOST or BV_MEM_DEVICE");
    const uint32_t n = mb->n_members;
    if (n && (!mb->data || !mb->member_off || !status)) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_inflate: null data/member_off/status");
    dst_off[0] = 0;
    if (n == 0) return BV_OK;
    std::vector<BvBgzfMember> hd;
    std::vector<uint8_t> pre;
    const int rc = bv_bgzf_headers(e, "bv_engine_bgzf_inflate", mb, hd, pre);
    if (rc != BV_OK) return rc;
    for (uint32_t k = 0; k < n; ++k) dst_off[k + 1] = dst_off[k] + hd[k].isize;
    if (dst_capacity < dst_off[n])
        return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_inflate: dst_capacity " + std::to_string(dst_capacity) + " < the " +
                                                         std::to_string(dst_off[n]) + " bytes the members inflate to");
    if (!dst && dst_off[n]) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_bgzf_inflate: null dst");
    return bgzf_inflate(e, state_of(e), mb, hd, pre, static_cast<uint8_t *>(dst), mem_kind == BV_MEM_HOST, dst_off, status, stream_ ? (hipStream_t)stream_ : e->stream);
}

}  // extern "C"
