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
#include <cstring>
#include <string>
#include <vector>

#include "../../include/basevar_amd_bgzf.h"
#include "bv_inflate_core.h"
#include "bv_chunk_stage.h"

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

// Per-engine staging of bv_engine_bgzf_inflate: the compressed chunks, each with its member table behind it (bv_chunk_stage.h
// has the rule of their reuse), and per slot a device chunk of inflated text for a host destination.
struct BvBgzfState {
    int device = 0;
    ChunkStage in;
    struct Slot {
        uint8_t *d_out = nullptr;  // written by the slot's kernel and copied back on the same stream: stream order keeps the next
        size_t out_cap = 0;        // chunk of the slot behind both, no event is needed
    } slot[2];
    uint8_t *d_status = nullptr;
    size_t status_cap = 0;
    bool lds_ok = false;  // the kernel's LDS was accepted
};

void bv_bgzf_state_free(BvBgzfState *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    chunk_stage_free(t->in);
    for (BvBgzfState::Slot &sl : t->slot)
        if (sl.d_out) (void)hipFree(sl.d_out);
    if (t->d_status) (void)hipFree(t->d_status);
    delete t;
}

namespace {

struct Chunk {
    uint32_t first, count;
    size_t in_bytes, out_bytes;
};

int bgzf_inflate(bv_engine *e, BvBgzfState *t, const bv_bgzf_members *mb, const std::vector<BvBgzfMember> &hd, const std::vector<uint8_t> &pre,
                 uint8_t *dst, bool host_dst, const uint64_t *out_pos, uint8_t *status, hipStream_t st) {
    const uint32_t n = mb->n_members;
    BV_HIP(e, hipSetDevice(t->device));
    int rc = chunk_stage_begin(e, t->in, st);
    if (rc == BV_OK)
        rc = kernel_lds_fits(e, "bv_engine_bgzf_inflate: the inflate kernel", reinterpret_cast<const void *>(bv_bgzf_inflate_kernel), t->device, &t->lds_ok);
    if (rc != BV_OK) return rc;
    const size_t in_cap = std::max<size_t>(chunk_limit_from_env("BASEVAR_AMD_TEXT_CHUNK_BYTES", kInChunkBytes), 65536);  // one member always fits
    const size_t out_cap = in_cap * kOutPerIn;
    std::vector<Chunk> chunks;
    size_t stage_max = 0, out_max = 0;
    for (uint32_t k = 0; k < n;) {
        Chunk c{k, 0, 0, 0};
        while (k < n && c.count < kChunkMembers) {
            const size_t len = mb->member_off[k + 1] - mb->member_off[k], text = hd[k].isize;
            if (c.count && (c.in_bytes + len > in_cap || c.out_bytes + text > out_cap)) break;
            c.in_bytes += len; c.out_bytes += text;
            ++c.count; ++k;
        }
        stage_max = std::max(stage_max, up16(c.in_bytes) + sizeof(BvInfMember) * c.count); out_max = std::max(out_max, c.out_bytes);
        chunks.push_back(c);
    }
    if ((rc = chunk_stage_reserve(e, t->in, stage_max)) != BV_OK) return rc;
    for (BvBgzfState::Slot &sl : t->slot)
        if ((rc = grow_device(e, &sl.d_out, &sl.out_cap, host_dst ? std::max<size_t>(out_max, 16) : 0)) != BV_OK) return rc;
    if ((rc = grow_device(e, &t->d_status, &t->status_cap, n)) != BV_OK) return rc;
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const Chunk &c = chunks[ci];
        const unsigned s = ci & 1u;
        if ((rc = chunk_stage_fill(e, t->in, s)) != BV_OK) return rc;
        // the members as they lie in the file, then their table
        uint8_t *h_in = t->in.slot[s].h;
        const size_t meta_at = up16(c.in_bytes);
        BvInfMember *h_meta = reinterpret_cast<BvInfMember *>(h_in + meta_at);
        size_t at = 0;
        for (uint32_t j = 0; j < c.count; ++j) {
            const uint32_t k = c.first + j;
            const size_t len = mb->member_off[k + 1] - mb->member_off[k];
            std::memcpy(h_in + at, mb->data + mb->member_off[k], len);
            BvInfMember &m = h_meta[j];
            m.out_off = host_dst ? out_pos[k] - out_pos[c.first] : out_pos[k];
            m.in_off = (uint32_t)(at + hd[k].payload_off); m.in_len = hd[k].payload_len;
            m.isize = hd[k].isize; m.crc = hd[k].crc; m.pre = pre[k]; m.reserved_ = 0;
            at += len;
        }
        if ((rc = chunk_stage_upload(e, t->in, s, meta_at + sizeof(BvInfMember) * c.count, st)) != BV_OK) return rc;
        const uint8_t *d_in = t->in.slot[s].d;
        uint8_t *d_out = t->slot[s].d_out;
        hipLaunchKernelGGL(bv_bgzf_inflate_kernel, dim3(c.count), dim3(64), 0, st, d_in, reinterpret_cast<const BvInfMember *>(d_in + meta_at), c.count,
                           host_dst ? d_out : dst, t->d_status + c.first);
        BV_HIP(e, hipGetLastError());
        if (host_dst && c.out_bytes)
            BV_HIP(e, hipMemcpyAsync(dst + out_pos[c.first], d_out, c.out_bytes, hipMemcpyDeviceToHost, st));
        if ((rc = chunk_stage_done(e, t->in, s, st)) != BV_OK) return rc;
    }
    BV_HIP(e, hipMemcpyAsync(status, t->d_status, n, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    return BV_OK;
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
    return bgzf_inflate(e, engine_state(e, e->bgzf), mb, hd, pre, d_dst, false, out_pos, status, st);
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
    return bgzf_inflate(e, engine_state(e, e->bgzf), mb, hd, pre, static_cast<uint8_t *>(dst), mem_kind == BV_MEM_HOST, dst_off, status, stream_ ? (hipStream_t)stream_ : e->stream);
}

}  // extern "C"
