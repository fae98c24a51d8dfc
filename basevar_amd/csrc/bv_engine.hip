// bv_engine.hip -- host side of the C ABI declared in include/basevar_amd.h: the engine's life cycle, stream ordering, the
// staging ring of host buffers, wait / timing / join, the host-log probe, NUMA placement and the synth entry point.  (Row
// submits: bv_engine_rows.hip; the tile mode: bv_engine_tiles.hip.)
//
// One engine = one HIP stream + the small device scratch the two passes share (phred
// tables, variant-site list, counters) + HIP events that time each pass on the stream it
// runs on.  No oracle, no CPU arithmetic path: if no HIP device or no gfx950 code object is
// usable, creation fails loudly with BV_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <link.h>
#include <sched.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "bv_engine_impl.h"
#ifdef BV_TEAM_DEBUG
#include "bv_engine_debug.h"
#endif

void bv_launch_synth(const bv_synth_params &p, uint32_t n_sites, uint32_t n_samples, uint64_t pitch, uint8_t *bs,
                     uint8_t *q, uint8_t *mapq, uint16_t *rpr, uint8_t *ref_base, hipStream_t stream);

namespace {
std::mutex g_err_mu;
std::string g_err;  // errors raised without an engine (create failures)

void set_global_error(const std::string &m) {
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_err = m;
}

// ---- the host libm's log() table (BvTables::hostlog, bv_log_host in bv_hostlog.h) ----------------------------------
// The reference's EM takes log() of per-sample marginals with the host's libm (algorithm.h:243) and compares /
// truncates sums of them; at tie-prone shallow sites the last bit of log() decides the call.  The device replays those
// sites with the host's own algorithm: its data table is looked up in the libm this process has loaded, and it is used
// only if the restated algorithm agrees with log() bit for bit on every probe below.  Anything else (another libm,
// another ifunc variant) leaves the table off and the device library's log in place -- correct, ulps from the host's.
struct HostLogFind {
    const double *tab;
};

int host_log_phdr_cb(struct dl_phdr_info *info, size_t, void *user) {
    // the C math library only: file name "libm.so*" or "libm-<version>.so" (not libmagma, libmpi, ...)
    if (!info->dlpi_name) return 0;
    const char *slash = std::strrchr(info->dlpi_name, '/');
    const char *fname = slash ? slash + 1 : info->dlpi_name;
    if (std::strncmp(fname, "libm.so", 7) != 0 && std::strncmp(fname, "libm-", 5) != 0) return 0;
    const double ln2hi = 0x1.62e42fefa3800p-1, ln2lo = 0x1.ef35793c76730p-45;  // the table opens with ln 2, split
    const size_t need = sizeof(double) * BV_HOSTLOG_N;
    for (int i = 0; i < info->dlpi_phnum; ++i) {
        const ElfW(Phdr) &ph = info->dlpi_phdr[i];
        if (ph.p_type != PT_LOAD || !(ph.p_flags & PF_R) || ph.p_memsz < need) continue;
        const char *base = reinterpret_cast<const char *>(info->dlpi_addr + ph.p_vaddr);
        for (size_t o = 0; o + need <= ph.p_memsz; o += 8) {
            double d[4];
            std::memcpy(d, base + o, sizeof d);
            if (d[0] == ln2hi && d[1] == ln2lo && d[2] < -0.49 && d[2] > -0.51 && d[3] > 0.33 && d[3] < 0.34) {
                static_cast<HostLogFind *>(user)->tab = reinterpret_cast<const double *>(base + o);
                return 1;
            }
        }
    }
    return 0;
}

inline uint64_t f64_bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}
inline double bits_f64(uint64_t u) {
    double x;
    std::memcpy(&x, &u, 8);
    return x;
}

// bv_log_host, on the host (same operations in the same order; std::fma is a true fused multiply-add)
double host_log_restated(double x, const double *T) {
    const double *A = T + 2, *B = T + 7, *tab = T + 18;
    uint64_t ix = f64_bits(x);
    const uint64_t LO = 0x3fee000000000000ull, HI = 0x3ff1090000000000ull;
    if (ix - LO < HI - LO) {
        if (ix == 0x3ff0000000000000ull) return 0.;
        const double r = x - 1.0, r2 = r * r, r3 = r * r2;
        const double pA = std::fma(r2, B[3], std::fma(r, B[2], B[1]));
        const double pB = std::fma(r2, B[6], std::fma(r, B[5], B[4]));
        const double pC = std::fma(r3, B[10], std::fma(r2, B[9], std::fma(r, B[8], B[7])));
        const double p = std::fma(std::fma(pC, r3, pB), r3, pA);
        const double t = std::fma(r, 0x1p27, r), rhi = std::fma(-0x1p27, r, t), rlo = r - rhi;
        const double s = rhi * rhi;
        const double hi = std::fma(s, B[0], r);
        const double lo = std::fma(s, B[0], r - hi);
        const double lo2 = std::fma(B[0] * rlo, rhi + r, lo);
        return std::fma(p, r3, lo2) + hi;
    }
    const uint32_t top = (uint32_t)(ix >> 48);
    if (top - 0x0010u >= 0x7ff0u - 0x0010u) {
        if ((ix << 1) == 0) return -HUGE_VAL;
        if (ix == 0x7ff0000000000000ull) return x;
        if ((top & 0x8000u) || (top & 0x7ff0u) == 0x7ff0u) return std::nan("");
        ix = f64_bits(x * 0x1p52);
        ix -= 52ull << 52;
    }
    const uint64_t tmp = ix - 0x3fe6000000000000ull;
    const uint32_t i = (uint32_t)(tmp >> 45) & 127u;
    const int k = (int)((int64_t)tmp >> 52);
    const double z = bits_f64(ix - (tmp & (0xfffull << 52)));
    const double invc = tab[2 * i], logc = tab[2 * i + 1], kd = (double)k;
    const double r = std::fma(z, invc, -1.0);
    const double w = std::fma(kd, T[0], logc), hi = r + w;
    const double lo = std::fma(kd, T[1], (w - hi) + r);
    const double r2 = r * r, r3 = r * r2;
    const double p = std::fma(std::fma(r, A[4], A[3]), r2, std::fma(r, A[2], A[1]));
    return std::fma(r3, p, std::fma(r2, A[0], lo)) + hi;
}

// fills dst[0..BV_HOSTLOG_N) + the "usable" flag behind it; true when the host's log() is reproduced exactly
bool load_host_log_table_once(double *dst);
// (searched and verified once per process: every engine gets a copy of the result)
bool load_host_log_table(double *dst) {
    static std::once_flag once;
    static double cached[BV_HOSTLOG_N + 2];
    static bool ok = false;
    std::call_once(once, [] { ok = load_host_log_table_once(cached); });
    std::memcpy(dst, cached, sizeof(cached));
    return ok;
}
bool load_host_log_table_once(double *dst) {
    std::memset(dst, 0, sizeof(double) * (BV_HOSTLOG_N + 2));
    HostLogFind find{nullptr};
    dl_iterate_phdr(host_log_phdr_cb, &find);
    if (!find.tab) return false;
    std::memcpy(dst, find.tab, sizeof(double) * BV_HOSTLOG_N);
    // probes: the marginals the EM sees are mixtures of (1 - eps_q) and eps_q / 3 -- those values, fractions of them,
    // a dense sweep of the near-1 branch, every table cell's two edges, and a spread of exponents down to subnormals
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
        return rng;
    };
    auto same = [&](double x) {
        volatile double vx = x;  // keep the compiler from folding log() of a constant
        const double a = host_log_restated(x, dst), b = std::log(vx);
        return f64_bits(a) == f64_bits(b) || (a != a && b != b);
    };
    bool ok = true;
    for (int qv = 0; qv < BV_QBINS && ok; ++qv) {
        const double eps = std::exp((double)qv * -0.23025850929940458);
        ok = ok && same(1.0 - eps) && same(eps / 3);
        for (int k = 1; k < 64 && ok; ++k) ok = same((1.0 - eps) * k / 64.0) && same(eps / 3 * k / 64.0) && same((1.0 - eps) * k / 64.0 + eps / 3 * (64 - k) / 64.0);
    }
    for (int n = 0; n < 200000 && ok; ++n) {
        const double u = (double)(next() >> 11) * 0x1p-53;                    // (0, 1)
        ok = same(u) && same(0.93 + 0.14 * u) && same(std::ldexp(0.5 + 0.5 * u, -(int)(next() % 1070)));
    }
    for (uint64_t i = 0; i < 128 && ok; ++i)
        for (int d = -2; d <= 2 && ok; ++d) ok = same(bits_f64(0x3fe6000000000000ull + (i << 45) + (uint64_t)(int64_t)d));
    ok = ok && same(5e-324) && same(2.0) && same(1e300) && same(0.0) && same(-1.0) && same(HUGE_VAL);
    dst[BV_HOSTLOG_N] = ok ? 1.0 : 0.0;
    return ok;
}
}  // namespace

int bv_impl::fail(bv_engine *e, int code, const std::string &msg) {
    if (e) {
        std::lock_guard<std::mutex> lk(e->mu);
        e->err = msg;
    } else {
        set_global_error(msg);
    }
    return code;
}
using namespace bv_impl;

// fold every completed pending triplet into the accumulators; `block` waits for them
int bv_impl::drain_timings(bv_engine *e, bool block) {
    while (e->ring_count > 0) {
        int slot = (e->ring_head - e->ring_count + bv_engine::kRing * 2) % bv_engine::kRing;
        hipEvent_t *t = e->ring[slot];
        if (block) {
            BV_HIP(e, hipEventSynchronize(t[2]));
        } else if (hipEventQuery(t[2]) != hipSuccess) {
            break;
        }
        float a = 0.f, b = 0.f, c = 0.f;
        BV_HIP(e, hipEventElapsedTime(&a, t[0], t[1]));
        BV_HIP(e, hipEventElapsedTime(&b, t[1], t[2]));
        if (e->ring_one_kernel[slot]) c = a;
        else BV_HIP(e, hipEventElapsedTime(&c, t[0], t[3]));
        e->acc1_ms += a;
        e->acc2_ms += b;
        e->acc_stream_ms += c;
        e->acc_n += 1;
        e->ring_count -= 1;
    }
    return BV_OK;
}

namespace {
// The engine's scratch (variant list, counters, staging) is shared by its submits, so work of one engine is
// serialised even when the caller alternates streams: a submit on a stream other than the previous one first
// waits for the end of the previous submit.  Every stream used is remembered for bv_engine_wait.
int flush_done(bv_engine *e) {
    if (e->done_pending) {
        BV_HIP(e, hipEventRecord(e->ev_done, e->done_stream));
        e->done_pending = false;
        e->ev_done_set = true;
    }
    return BV_OK;
}
}  // namespace

namespace bv_impl {
int use_stream(bv_engine *e, hipStream_t st) {
    bool seen = false;
    for (hipStream_t u : e->used_streams) seen |= (u == st);
    if (!seen) e->used_streams.push_back(st);
    if (st != e->last_stream) {
        int rc = flush_done(e);
        if (rc != BV_OK) return rc;
        if (e->ev_done_set) BV_HIP(e, hipStreamWaitEvent(st, e->ev_done, 0));
    }
    e->last_stream = st;
    return BV_OK;
}
// The end of a submit is marked lazily: the event is recorded only when somebody needs it -- a submit on another stream,
// bv_engine_join -- and then on the stream that carried the submit (whatever the caller queued there since is waited for too:
// conservative, never wrong).  A host that keeps to one stream pays for no event at all (an event record behind every submit
// was one more packet in front of the next submit's first kernel).
int mark_done(bv_engine *e, hipStream_t st) {
    e->done_pending = true;
    e->done_stream = st;
    return BV_OK;
}
// group ids as the kernels read them: 16-byte chunks up to round_up(n_samples, 16) -- the ABI promises only
// [n_samples] bytes of any alignment, so the engine keeps its own padded copy (n_samples bytes per submit)
int stage_group_ids(bv_engine *e, const uint8_t *gid, uint32_t n_samples, bool host, hipStream_t st, const uint8_t **out) {
    const size_t need = up256(n_samples) + 256;
    const int rc = grow_device(e, &e->d_gid, &e->d_gid_bytes, need);
    if (rc != BV_OK) return rc;
    BV_HIP(e, hipMemsetAsync(e->d_gid, 0xFF, need, st));
    BV_HIP(e, hipMemcpyAsync(e->d_gid, gid, n_samples, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    *out = e->d_gid;
    return BV_OK;
}
// ---- staging ring
int stage_acquire(bv_engine *e, size_t bytes, StageSlot **out) {
    for (auto &cs : e->copy_stream)
        if (!cs) BV_HIP(e, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    const unsigned k = e->sring_next++;
    StageSlot &sl = e->sring[k % bv_engine::kStage];
    sl.cs = e->copy_stream[k & 1u];
    if (!sl.copied) {
        BV_HIP(e, hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming));
        BV_HIP(e, hipEventCreateWithFlags(&sl.freed, hipEventDisableTiming));
    }
    if (bytes > sl.bytes) sl.used = false;  // a new buffer: nothing reads it yet
    const int rc = grow_device(e, &sl.buf, &sl.bytes, bytes);
    if (rc != BV_OK) return rc;
    // the buffer is free again once the work that read it last has run
    if (sl.used) BV_HIP(e, hipStreamWaitEvent(sl.cs, sl.freed, 0));
    *out = &sl;
    return BV_OK;
}
// BV_FLAG_HOST_ORDERED: the copies of host planes wait for everything queued on the caller's stream so far (a caller that
// fills its pinned planes with asynchronous work on that stream).  Default: host planes are complete when the call is made
// (include/basevar_amd.h) and the copy runs ahead, under the kernels of earlier submits.
int stage_order(bv_engine *e, StageSlot *sl, hipStream_t st) {
    if (!(e->cfg.flags & BV_FLAG_HOST_ORDERED)) return BV_OK;
    if (!e->ev_host) BV_HIP(e, hipEventCreateWithFlags(&e->ev_host, hipEventDisableTiming));
    BV_HIP(e, hipEventRecord(e->ev_host, st));
    BV_HIP(e, hipStreamWaitEvent(sl->cs, e->ev_host, 0));
    return BV_OK;
}
int stage_publish(bv_engine *e, StageSlot *sl, hipStream_t st) {  // the copies are queued: `st` may read after them
    BV_HIP(e, hipEventRecord(sl->copied, sl->cs));
    BV_HIP(e, hipStreamWaitEvent(st, sl->copied, 0));
    return BV_OK;
}
int stage_release(bv_engine *e, StageSlot *sl, hipStream_t st) {  // everything queued on `st` so far is the last reader
    BV_HIP(e, hipEventRecord(sl->freed, st));
    sl->used = true;
    return BV_OK;
}
// Host planes that lie in ONE allocation, one after the other (a packed tile, see bv_tile_packed_layout), go over the
// link as one copy: the per-copy cost of five 2-3 MB copies per tile was a quarter of the tile's transfer time.
HostPlanes plan_host_planes(const HostPlane *pl, int n) {
    HostPlanes h;
    size_t sum = 0;
    for (int i = 0; i < n; ++i) {
        if (!pl[i].src || !pl[i].bytes) continue;
        const uint8_t *a = static_cast<const uint8_t *>(pl[i].src);
        if (!h.lo || a < h.lo) h.lo = a;
        if (!h.hi || a + pl[i].bytes > h.hi) h.hi = a + pl[i].bytes;
        sum += up256(pl[i].bytes);
    }
    // ONE copy only for the exact layout of bv_tile_packed_layout: the planes in order, each at the 256-aligned end of the one
    // before it, in one allocation -- then every byte of [lo, hi) is the caller's.  (Planes that merely lie close together
    // are copied one by one: the bytes between them are not ours to read.)
    bool one_copy = h.lo != nullptr && (reinterpret_cast<uintptr_t>(h.lo) & 15u) == 0;
    {
        size_t at = 0;
        for (int i = 0; i < n && one_copy; ++i) {
            if (!pl[i].src || !pl[i].bytes) continue;
            one_copy = static_cast<const uint8_t *>(pl[i].src) == h.lo + at;
            at += up256(pl[i].bytes);
        }
    }
    h.one_copy = one_copy;
    h.bytes = one_copy ? up256((size_t)(h.hi - h.lo)) : sum;
    return h;
}
int copy_host_planes(bv_engine *e, HostPlane *pl, int n, const HostPlanes &h, uint8_t *base, hipStream_t cs) {
    if (h.one_copy) {
        BV_HIP(e, hipMemcpyAsync(base, h.lo, (size_t)(h.hi - h.lo), hipMemcpyHostToDevice, cs));
        for (int i = 0; i < n; ++i)
            pl[i].dev = (pl[i].src && pl[i].bytes) ? base + (static_cast<const uint8_t *>(pl[i].src) - h.lo) : nullptr;
    } else {
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            pl[i].dev = nullptr;
            if (!pl[i].src || !pl[i].bytes) continue;
            BV_HIP(e, hipMemcpyAsync(base + off, pl[i].src, pl[i].bytes, hipMemcpyHostToDevice, cs));
            pl[i].dev = base + off;
            off += up256(pl[i].bytes);
        }
    }
    return BV_OK;
}
int stage_host_planes(bv_engine *e, HostPlane *pl, int n, size_t extra, StageSlot **slot_out, uint8_t **extra_dev, hipStream_t st) {
    const HostPlanes h = plan_host_planes(pl, n);
    StageSlot *sl = nullptr;
    int rc = stage_acquire(e, h.bytes + up256(extra), &sl);
    if (rc != BV_OK) return rc;
    rc = stage_order(e, sl, st);
    if (rc != BV_OK) return rc;
    uint8_t *base = static_cast<uint8_t *>(sl->buf);
    rc = copy_host_planes(e, pl, n, h, base, sl->cs);
    if (rc != BV_OK) return rc;
    *slot_out = sl;
    if (extra_dev) *extra_dev = base + h.bytes;
    return BV_OK;
}
int stage_records(bv_engine *e, HostPlane *pl, int n, size_t S, size_t G, bv_site_result *out, bv_group_result *gout, StageSlot **slot,
                  bv_site_result **dout, bv_group_result **dgout, hipStream_t st) {
    const size_t out_b = up256(S * sizeof(bv_site_result)), gout_b = up256(S * G * sizeof(bv_group_result));
    uint8_t *extra = nullptr;
    int rc = stage_host_planes(e, pl, n, out_b + gout_b, slot, &extra, st);
    if (rc != BV_OK) return rc;
    rc = stage_publish(e, *slot, st);
    if (rc != BV_OK) return rc;
    *dout = reinterpret_cast<bv_site_result *>(extra);
    *dgout = G ? reinterpret_cast<bv_group_result *>(extra + out_b) : nullptr;
    e->stage_out = *dout; e->stage_gout = *dgout;
    e->host_out = out; e->host_gout = gout;
    e->host_out_bytes = S * sizeof(bv_site_result);
    e->host_gout_bytes = S * G * sizeof(bv_group_result);
    return BV_OK;
}
int copy_records_back(bv_engine *e, hipStream_t st) {
    if (!e->host_out) return BV_OK;
    BV_HIP(e, hipMemcpyAsync(e->host_out, e->stage_out, e->host_out_bytes, hipMemcpyDeviceToHost, st));
    if (e->host_gout && e->host_gout_bytes)
        BV_HIP(e, hipMemcpyAsync(e->host_gout, e->stage_gout, e->host_gout_bytes, hipMemcpyDeviceToHost, st));
    return BV_OK;
}
}  // namespace bv_impl

extern "C" {

const char *bv_version(void) { return "basevar_amd 0.2 abi2 gfx950"; }

double bv_min_af(uint32_t n_samples, float user_min_af) {
    // src/basetype_caller.cpp:122: min_af = std::min(float(100)/input_bf.size(), min_af)
    float a = float(100) / n_samples;
    float m = (a < user_min_af) ? a : user_min_af;
    return (double)m;
}

int bv_engine_create(const bv_engine_config *cfg, bv_engine **out) {
    if (!cfg || !out) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_create: null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, BV_ERR_NO_DEVICE, "bv_engine_create: no HIP device visible (the engine has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_create: device ordinal out of range");
    if (cfg->max_sites == 0) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_create: max_sites == 0");
    // the fault-injection bit (basevar_amd_diag.h) makes every launch stall ~2 s and fail: refused unless the process asks for it
    if ((cfg->flags & BV_FLAG_FAULT_LOST_HANDOFF) && !std::getenv("BASEVAR_AMD_FAULT_INJECT"))
        return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_create: BV_FLAG_FAULT_LOST_HANDOFF is a test-only fault injection; set BASEVAR_AMD_FAULT_INJECT=1 to allow it");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
        return fail(nullptr, BV_ERR_NO_DEVICE, "bv_engine_create: cannot query device");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, BV_ERR_NO_DEVICE,
                    std::string("bv_engine_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);

    bv_engine *e = new bv_engine();
    e->cfg = *cfg;
    auto bail = [&](int code) {
        std::string m = e->err;
        bv_engine_destroy(e);
        set_global_error(m);
        return code;
    };
#define BV_TRY(call)                                                                                  \
    do {                                                                                              \
        hipError_t _s = (call);                                                                       \
        if (_s != hipSuccess) {                                                                       \
            e->err = std::string(#call) + ": " + hipGetErrorString(_s);                               \
            return bail(BV_ERR_HIP);                                                                  \
        }                                                                                             \
    } while (0)
    BV_TRY(hipSetDevice(cfg->device));
    e->n_cu = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
    BV_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    BV_TRY(hipEventCreateWithFlags(&e->ev_done, hipEventDisableTiming));
    for (auto &tri : e->ring)
        for (auto &ev : tri) BV_TRY(hipEventCreate(&ev));
    BV_TRY(hipMalloc(&e->d_tables, sizeof(BvTables)));
    BV_TRY(hipMalloc(&e->d_var_list, sizeof(uint32_t) * (size_t)cfg->max_sites));
    BV_TRY(hipMalloc(&e->d_counters, sizeof(uint32_t) * BV_CTR_WORDS * bv_engine::kCtrBlocks));
    BV_TRY(hipHostMalloc(&e->h_counters, sizeof(uint32_t) * BV_CTR_WORDS * bv_engine::kCtrBlocks));
    std::memset(e->h_counters, 0, sizeof(uint32_t) * BV_CTR_WORDS * bv_engine::kCtrBlocks);
    BV_TRY(hipMemset(e->d_counters, 0, sizeof(uint32_t) * BV_CTR_WORDS * bv_engine::kCtrBlocks));

    // eps table with the host libm, exactly the reference's expression (basetype.cpp:47-48, :63)
    BvTables t;
    const double MLN10TO10 = -0.23025850929940458;  // basetype.h:20
    for (int qv = 0; qv < BV_QBINS; ++qv) {
        double epsilon = exp((double)qv * MLN10TO10);
        t.hit[qv] = 1.0 - epsilon;
        t.miss[qv] = epsilon / 3;
        // log of the two likelihood values with the host libm (algorithm.h:243 takes log of exactly these when a
        // subset holds one base); log(0) = -inf at phred 0 is never read (such sites take the iterative path)
        t.loghit[qv] = log(t.hit[qv]);
        t.logmiss[qv] = log(t.miss[qv]);
    }
    e->host_log_exact = load_host_log_table(t.hostlog) ? 1 : 0;
    if (!e->host_log_exact) {
        // not silent: said once per process on stderr, kept as the global message (bv_last_error(NULL)) of this successful
        // create, and flagged per record (BV_SITE_LOG_APPROX) on the sites it concerns
        static const char *note =
            "basevar_amd: note: the host libm's log() could not be reproduced on the device (no glibc __log_data table found, or it "
            "failed verification); sites of <= 64 covered samples use the device library's log(): values within 1e-6, exact ties "
            "between allele subsets undecided (records carry BV_SITE_LOG_APPROX)";
        static std::once_flag said;
        std::call_once(said, [] { if (!std::getenv("BASEVAR_AMD_QUIET")) std::fprintf(stderr, "%s\n", note); });
        set_global_error(note);
    }
    // log-factorials for the Fisher test with the host libm -- kfunc.c:197-201 calls lgamma(n + 1) --
    // for every depth a site of this engine can reach (deeper tables fall back to a series on the device)
    {
        size_t nfact = (size_t)(cfg->max_samples ? cfg->max_samples : 1u << 20) + 2;
        if (nfact < (1u << 16)) nfact = 1u << 16;
        if (nfact > (1u << 23)) nfact = 1u << 23;
        std::vector<double> lf(nfact);
        for (size_t k = 0; k < nfact; ++k) {
            int sign;
            lf[k] = lgamma_r((double)k + 1.0, &sign);
        }
        BV_TRY(hipMalloc(&e->d_lnfact, sizeof(double) * nfact));
        BV_TRY(hipMemcpy(e->d_lnfact, lf.data(), sizeof(double) * nfact, hipMemcpyHostToDevice));
        t.lnfact = e->d_lnfact;
        t.lnfact_n = (uint32_t)nfact;
        t.pad_ = 0;
    }
    BV_TRY(hipMemcpy(e->d_tables, &t, sizeof(t), hipMemcpyHostToDevice));
#undef BV_TRY
    if (cfg->flags & BV_FLAG_LANES) {
        // the two lanes now, not at their first submit: a process has few hardware queues and streams are dealt to them in
        // the order they are created -- created late, the lanes landed on queues already carrying other streams
        if (const char *nl = std::getenv("BASEVAR_AMD_LANES")) e->n_lanes = std::max(2, std::min((int)bv_engine::kMaxLanes, std::atoi(nl)));
        for (int k = 0; k < e->n_lanes; ++k) {
            bv_engine_config c = *cfg;
            c.flags &= ~BV_FLAG_LANES;
            const int rc = bv_engine_create(&c, &e->lane[k]);
            if (rc != BV_OK) {
                const std::string m = bv_last_error(nullptr);
                bv_engine_destroy(e);
                set_global_error("bv_engine_create: lane engine: " + m);
                return rc;
            }
            e->lane[k]->is_lane = true;
        }
    }
    *out = e;
    return BV_OK;
}

int bv_engine_destroy(bv_engine *e) {
    if (!e) return BV_OK;
    (void)hipSetDevice(e->cfg.device);
    for (bv_engine *&l : e->lane) {
        if (l) (void)bv_engine_destroy(l);
        l = nullptr;
    }
    if (e->ev_entry) (void)hipEventDestroy(e->ev_entry);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    bv_text_state_free(e->text);
    bv_bgzf_state_free(e->bgzf);
    bv_deflate_state_free(e->deflate);
    bv_vcf_state_free(e->vcf);
    bv_pileup_state_free(e->pileup);
    bv_ptext_state_free(e->ptext);
    bv_rtext_state_free(e->rtext);
    bv_indel_state_free(e->indel);
    bv_text_tok_state_free(e->ttok);
    for (hipStream_t st : e->used_streams) (void)hipStreamSynchronize(st);
    for (auto &tri : e->ring)
        for (auto &ev : tri)
            if (ev) (void)hipEventDestroy(ev);
    if (e->d_tables) (void)hipFree(e->d_tables);
    if (e->d_lnfact) (void)hipFree(e->d_lnfact);
    if (e->d_var_list) (void)hipFree(e->d_var_list);
    if (e->d_counters) (void)hipFree(e->d_counters);
    if (e->d_gid) (void)hipFree(e->d_gid);
    row_scratch_free(e);
    if (e->ev_done) (void)hipEventDestroy(e->ev_done);
    if (e->ev_host) (void)hipEventDestroy(e->ev_host);
    if (e->h_counters) (void)hipHostFree(e->h_counters);
    for (auto &sl : e->sring) {
        if (sl.buf) (void)hipFree(sl.buf);
        if (sl.copied) (void)hipEventDestroy(sl.copied);
        if (sl.freed) (void)hipEventDestroy(sl.freed);
    }
    tile_job_free(e->tile);
    for (hipStream_t cs : e->copy_stream)
        if (cs) (void)hipStreamSynchronize(cs);
    for (hipStream_t cs : e->copy_stream)
        if (cs) (void)hipStreamDestroy(cs);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return BV_OK;
}

void *bv_engine_stream(bv_engine *e) { return e ? (void *)e->stream : nullptr; }

int bv_engine_wait(bv_engine *e) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_wait: null engine");
    if (!e->submitted) return BV_OK;
    BV_HIP(e, hipSetDevice(e->cfg.device));
    for (bv_engine *l : e->lane) {
        if (!l) continue;
        const int rc = bv_engine_wait(l);
        if (rc != BV_OK) return fail(e, rc, bv_last_error(l));
    }
    if (e->last_stream == nullptr && e->used_streams.empty()) return BV_OK;  // only lanes carried work
    // every stream that carried a submit since the last wait (submits of one engine are serialised through ev_done,
    // so the counters mirrored by the LAST submit are final once all of them have drained)
    for (hipStream_t st : e->used_streams) BV_HIP(e, hipStreamSynchronize(st));
    e->used_streams.clear();
    e->used_streams.push_back(e->last_stream);
    e->done_pending = false; e->ev_done_set = false;  // everything submitted so far has finished: nothing left to order behind
    if (e->ctr_mirror_stale) {  // (the streams are idle: a plain copy)
        BV_HIP(e, hipMemcpy(e->h_counters, e->d_counters, sizeof(uint32_t) * BV_CTR_WORDS * bv_engine::kCtrBlocks, hipMemcpyDeviceToHost));
        e->ctr_mirror_stale = false;
    }
    uint32_t timed_out = 0, zero_freq = 0;
    for (uint32_t b = 0; b < bv_engine::kCtrBlocks; ++b) {
#ifdef BV_TEAM_DEBUG
        if (b == 0 && e->h_counters[BV_CTR_WORDS + 5150] == 1u) bv_stream_debug_report(e->h_counters);
        else if (b == 0 && e->h_counters[BV_CTR_WORDS + 5150] == 2u) bv_team_debug_report(e->h_counters);
        else if (b == 0 && e->h_counters[BV_CTR_WORDS + 5150] == 4u) bv_fused_debug_report(e->h_counters);
#endif
        timed_out |= e->h_counters[(size_t)b * BV_CTR_WORDS + BV_CTR_TIMEOUT];  // bit-coded BV_TMO_* flags, ORed by the kernels: OR here too
        zero_freq += e->h_counters[(size_t)b * BV_CTR_WORDS + BV_CTR_ZEROFREQ];
    }
    if (timed_out != 0 || zero_freq != 0) {
        // the error counters are sticky on the device (they accumulate over submits): reported once, then cleared
        for (uint32_t b = 0; b < bv_engine::kCtrBlocks; ++b) {
            BV_HIP(e, hipMemsetAsync(e->d_counters + (size_t)b * BV_CTR_WORDS + BV_CTR_PER_LAUNCH * BV_CTR_STRIDE, 0,
                                     sizeof(uint32_t) * (BV_CTR_WORDS - BV_CTR_PER_LAUNCH * BV_CTR_STRIDE), e->last_stream));
            e->h_counters[(size_t)b * BV_CTR_WORDS + BV_CTR_TIMEOUT] = e->h_counters[(size_t)b * BV_CTR_WORDS + BV_CTR_ZEROFREQ] = 0;
        }
        BV_HIP(e, hipStreamSynchronize(e->last_stream));
    }
    if (timed_out != 0) {
        char buf[200];
        std::snprintf(buf, sizeof buf, "pass 1: an intra-workgroup hand-off timed out (internal error; results invalid; which: %#x, see BV_TMO_* in "
                                       "csrc/bv_kernels.h)", timed_out);
        return fail(e, BV_ERR_HIP, buf);
    }
    if (zero_freq > 0) {
        char buf[160];
        std::snprintf(buf, sizeof buf,
                      "The sum of frequence of active bases must always > 0 (%u site(s); see BV_SITE_ZERO_FREQ)", zero_freq);
        return fail(e, BV_ERR_SITE, buf);  // message of src/basetype.cpp:114
    }
    return BV_OK;
}

int bv_engine_kernel_ms(bv_engine *e, float *pass1_ms, float *pass2_ms) {
    if (!e || !e->submitted) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_kernel_ms: nothing submitted");
    if (e->last_lane >= 0) return bv_engine_kernel_ms(e->lane[e->last_lane], pass1_ms, pass2_ms);
    if (e->last_slot < 0)
        return fail(e, BV_ERR_INVALID_ARG, "bv_engine_kernel_ms: the last job recorded no pass timings (per-site-tally tile job)");
    float a = 0.f, b = 0.f;
    hipEvent_t *t = e->ring[e->last_slot];
    BV_HIP(e, hipEventSynchronize(t[2]));
    BV_HIP(e, hipEventElapsedTime(&a, t[0], t[1]));
    BV_HIP(e, hipEventElapsedTime(&b, t[1], t[2]));
    if (pass1_ms) *pass1_ms = a;
    if (pass2_ms) *pass2_ms = b;
    return BV_OK;
}

int bv_engine_timing_reset(bv_engine *e) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_timing_reset: null engine");
    BV_HIP(e, hipSetDevice(e->cfg.device));
    int rc = drain_timings(e, true);
    if (rc != BV_OK) return rc;
    e->acc1_ms = e->acc2_ms = e->acc_stream_ms = 0.;
    e->acc_n = 0;
    for (bv_engine *l : e->lane)
        if (l && (rc = bv_engine_timing_reset(l)) != BV_OK) return rc;
    return BV_OK;
}

int bv_engine_timing_get(bv_engine *e, double *pass1_total_ms, double *pass2_total_ms, uint32_t *n_submits) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_timing_get: null engine");
    BV_HIP(e, hipSetDevice(e->cfg.device));
    int rc = drain_timings(e, true);
    if (rc != BV_OK) return rc;
    double a1 = e->acc1_ms, a2 = e->acc2_ms;
    uint32_t an = e->acc_n;
    for (bv_engine *l : e->lane) {  // the lanes' submits are this engine's
        if (!l) continue;
        double x = 0, y = 0; uint32_t m = 0;
        if ((rc = bv_engine_timing_get(l, &x, &y, &m)) != BV_OK) return rc;
        a1 += x; a2 += y; an += m;
    }
    if (pass1_total_ms) *pass1_total_ms = a1;
    if (pass2_total_ms) *pass2_total_ms = a2;
    if (n_submits) *n_submits = an;
    return BV_OK;
}

int bv_engine_timing_get_ex(bv_engine *e, double *stream_total_ms, double *pass1_total_ms, double *pass2_total_ms,
                            uint32_t *n_submits) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_timing_get_ex: null engine");
    BV_HIP(e, hipSetDevice(e->cfg.device));
    int rc = drain_timings(e, true);
    if (rc != BV_OK) return rc;
    double as = e->acc_stream_ms, a1 = e->acc1_ms, a2 = e->acc2_ms;
    uint32_t an = e->acc_n;
    for (bv_engine *l : e->lane) {
        if (!l) continue;
        double w = 0, x = 0, y = 0; uint32_t m = 0;
        if ((rc = bv_engine_timing_get_ex(l, &w, &x, &y, &m)) != BV_OK) return rc;
        as += w; a1 += x; a2 += y; an += m;
    }
    if (stream_total_ms) *stream_total_ms = as;
    if (pass1_total_ms) *pass1_total_ms = a1;
    if (pass2_total_ms) *pass2_total_ms = a2;
    if (n_submits) *n_submits = an;
    return BV_OK;
}

// Make `stream` wait for every submit issued so far.  Without BV_FLAG_LANES the submits already ran on the stream they
// were given; with it they run on the lanes' own streams and a consumer ordered on a stream (a gather of the records,
// a copy) calls this first.
int bv_engine_join(bv_engine *e, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_join: null engine");
    BV_HIP(e, hipSetDevice(e->cfg.device));
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    for (bv_engine *l : e->lane) {
        if (!l) continue;
        int rc = flush_done(l);
        if (rc != BV_OK) return fail(e, rc, bv_last_error(l));
        if (l->ev_done_set) BV_HIP(e, hipStreamWaitEvent(st, l->ev_done, 0));
    }
    if (st != e->last_stream) {
        int rc = flush_done(e);
        if (rc != BV_OK) return rc;
        if (e->ev_done_set) BV_HIP(e, hipStreamWaitEvent(st, e->ev_done, 0));
    }
    return BV_OK;
}

int bv_host_log_probe(double *table) {
    double t[BV_HOSTLOG_N + 2];
    const bool ok = load_host_log_table(t);
    if (ok && table) std::memcpy(table, t, sizeof(double) * BV_HOSTLOG_N);
    return ok ? 1 : 0;
}

double bv_host_log_eval(const double *table, double x) { return host_log_restated(x, table); }

int bv_engine_host_log_exact(const bv_engine *e) { return e ? e->host_log_exact : 0; }

__global__ void bv_host_log_eval_kernel(const BvTables *tables, const double *x, double *y, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = bv_log_host(x[i], tables->hostlog);
}

int bv_engine_host_log_eval(bv_engine *e, const double *x, double *y, uint32_t n) {
    if (!e || !x || !y) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_host_log_eval: null argument");
    if (!e->host_log_exact) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_host_log_eval: the host log table was not verified on this host");
    if (n == 0) return BV_OK;
    BV_HIP(e, hipSetDevice(e->cfg.device));
    double *d = nullptr;
    BV_HIP(e, hipMalloc(&d, sizeof(double) * 2 * (size_t)n));
    hipError_t st = hipMemcpy(d, x, sizeof(double) * n, hipMemcpyHostToDevice);
    if (st == hipSuccess) {
        bv_host_log_eval_kernel<<<(n + 255u) / 256u, 256, 0, e->stream>>>(e->d_tables, d, d + n, n);
        st = hipGetLastError();
    }
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    if (st == hipSuccess) st = hipMemcpy(y, d + n, sizeof(double) * n, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (st != hipSuccess) return fail(e, BV_ERR_HIP, std::string("bv_engine_host_log_eval: ") + hipGetErrorString(st));
    return BV_OK;
}

int bv_engine_last_launch_form(bv_engine *e, uint32_t *form) {
    if (!e || !form) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_last_launch_form: null argument");
    if (e->last_lane >= 0) return bv_engine_last_launch_form(e->lane[e->last_lane], form);
    *form = e->last_form;
    return BV_OK;
}

int bv_engine_last_variant_count(bv_engine *e, uint32_t *n_variant) {
    if (!e || !n_variant) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_last_variant_count: null argument");
    if (e->last_lane >= 0) return bv_engine_last_variant_count(e->lane[e->last_lane], n_variant);
    *n_variant = e->h_counters[(size_t)e->last_ctr_base * BV_CTR_WORDS + BV_CTR_VARIANTS];
    return BV_OK;
}

const char *bv_last_error(const bv_engine *e) {
    static thread_local std::string copy;
    if (e) {
        std::lock_guard<std::mutex> lk(e->mu);
        copy = e->err;
    } else {
        std::lock_guard<std::mutex> lk(g_err_mu);
        copy = g_err;
    }
    return copy.c_str();
}

// ---- NUMA placement of host buffers ---------------------------------------------------------------------------------
// The node a GPU's PCIe function hangs off, from sysfs (hipDeviceGetPCIBusId -> /sys/bus/pci/devices/<bdf>/numa_node).
int bv_device_numa_node(int device, char *pci_bdf, size_t pci_bdf_len) {
    char bdf[32] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    for (char *c = bdf; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
    if (pci_bdf && pci_bdf_len) std::snprintf(pci_bdf, pci_bdf_len, "%s", bdf);
    char path[128];
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
    int node = -1;
    if (FILE *f = std::fopen(path, "r")) {
        if (std::fscanf(f, "%d", &node) != 1) node = -1;
        std::fclose(f);
    }
    return node;
}

// The calling thread keeps those of its CPUs that belong to the GPU's node: memory it allocates and first touches from now on
// (pinned tiles, staging vectors) is node-local under the default policy.  Returns the node, or -1 with the mask unchanged
// (no node reported, no node CPU list, or none of the node's CPUs in the current mask).
int bv_bind_thread_to_device_node(int device) {
    const int node = bv_device_numa_node(device, nullptr, 0);
    if (node < 0) return -1;
    char path[128];
    std::snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = std::fopen(path, "r");
    if (!f) return -1;
    char buf[4096] = {0};
    const size_t got = std::fread(buf, 1, sizeof buf - 1, f);
    std::fclose(f);
    buf[got] = 0;
    cpu_set_t cur, want;
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof cur, &cur) != 0) return -1;
    int n_set = 0;
    char *save = nullptr;  // (strtok_r: bv_call's per-GPU worker threads bind themselves concurrently)
    for (char *tok = strtok_r(buf, ",\n", &save); tok; tok = strtok_r(nullptr, ",\n", &save)) {  // "0-63,128-191"
        int lo = 0, hi = 0;
        const int k = std::sscanf(tok, "%d-%d", &lo, &hi);
        if (k < 1) continue;
        if (k == 1) hi = lo;
        for (int c = lo; c <= hi && c < CPU_SETSIZE; ++c)
            if (CPU_ISSET(c, &cur)) { CPU_SET(c, &want); ++n_set; }
    }
    if (n_set == 0) return -1;
    if (sched_setaffinity(0, sizeof want, &want) != 0) return -1;
    return node;
}

int bv_synth_fill(int device, const bv_synth_params *p, uint32_t n_sites, uint32_t n_samples, uint64_t pitch,
                  uint8_t *base_strand, uint8_t *qual, uint8_t *mapq, uint16_t *rpr, uint8_t *ref_base, void *stream) {
    if (!p || !base_strand || !qual || !ref_base || n_sites == 0 || n_samples == 0 || pitch < n_samples || (pitch & 15ull))
        return fail(nullptr, BV_ERR_INVALID_ARG, "bv_synth_fill: bad argument");
    BV_HIP(nullptr, hipSetDevice(device));
    bv_launch_synth(*p, n_sites, n_samples, pitch, base_strand, qual, mapq, rpr, ref_base, (hipStream_t)stream);
    BV_HIP(nullptr, hipGetLastError());
    return BV_OK;
}

}  // extern "C"
