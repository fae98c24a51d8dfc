// bv_chunk_stage.h -- host bytes to the device, a chunk at a time, under the kernels that read the chunk before: what
// bv_text.hip (rows of text), bv_inflate.hip (BGZF members) and bv_deflate.hip (blocks of text) share.  Host-only.
//
// A ChunkStage is two slots and a copy stream `cs` of its own.  A slot is a pinned host chunk `h`, a device chunk `d` of the
// same capacity, and two events.  Chunk k of a call goes through slot k & 1:
//
//     chunk_stage_fill(s)              the host may write slot s's `h`
//     ... the caller writes the chunk's bytes to `h`: the data, and behind it (16-byte aligned) whatever small tables the kernel
//         reads with it, so that ONE copy takes both over the link ...
//     chunk_stage_upload(s, bytes, st) h -> d on `cs`; `st` waits for the copy
//     ... the caller queues the chunk's kernels (and copies back) on `st` ...
//     chunk_stage_done(s, st)          what `st` holds now is the last reader of slot s
//
// THE REUSE RULE, the same for every user:
//   - `h` of slot s is free once `copied[s]` has passed (its bytes have crossed the link): the HOST waits for it, in
//     chunk_stage_fill.
//   - `d` of slot s is free once `done[s]` has passed (the kernels that read it are through): the COPY STREAM waits for it, in
//     chunk_stage_upload; the host does not.  So the host packs chunk k + 2 while the kernels of chunk k still run.
//   - `back` of slot s (optional: pinned bytes that a copy on `st`, queued before chunk_stage_done, brings back) may be read by
//     the host after chunk_stage_wait_done(s).  A caller that reads it does so before it fills the slot again.
//   - What a caller keeps per slot on the device and touches on `st` alone (written by the chunk's kernels, copied back on `st`)
//     needs no event: stream order keeps chunk k + 2 behind chunk k.
// Every call begins with chunk_stage_begin, which waits for `cs` and `st`: a call that failed part-way may have left work
// queued, and the staging is free only once that is through.
#pragma once

#include <cstdlib>

#include "bv_engine_impl.h"

namespace bv_impl {

struct ChunkStage {
    hipStream_t cs = nullptr;  // the copy stream of the chunks
    struct Slot {
        uint8_t *h = nullptr, *d = nullptr;
        uint8_t *back = nullptr;  // behind `h`, in its allocation
        hipEvent_t copied = nullptr, done = nullptr;
        bool used = false;  // the events have been recorded
    } slot[2];
    size_t cap = 0, back_cap = 0;  // bytes of every h / d, of every back (0 until all of them exist)
};

// The stream and the events, each if it is missing (a call that failed half-way is taken up where it stopped); then the entry
// guard: nothing of an earlier call is left on `cs` or `st`.
inline int chunk_stage_begin(bv_engine *e, ChunkStage &c, hipStream_t st) {
    if (!c.cs) BV_HIP(e, hipStreamCreateWithFlags(&c.cs, hipStreamNonBlocking));
    for (ChunkStage::Slot &sl : c.slot) {
        if (!sl.copied) BV_HIP(e, hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming));
        if (!sl.done) BV_HIP(e, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    BV_HIP(e, hipStreamSynchronize(c.cs));
    BV_HIP(e, hipStreamSynchronize(st));
    return BV_OK;
}

// Chunks of at least `bytes` (and `back_bytes` to come back, behind them in the same pinned allocation); they only grow.  After
// chunk_stage_begin: nothing uses them.
inline int chunk_stage_reserve(bv_engine *e, ChunkStage &c, size_t bytes, size_t back_bytes = 0) {
    if (bytes <= c.cap && back_bytes <= c.back_cap) return BV_OK;
    bytes = bytes > c.cap ? bytes : c.cap;
    back_bytes = back_bytes > c.back_cap ? back_bytes : c.back_cap;
    c.cap = c.back_cap = 0;
    for (ChunkStage::Slot &sl : c.slot) {
        if (sl.h) BV_HIP(e, hipHostFree(sl.h));
        sl.h = sl.back = nullptr;
        if (sl.d) BV_HIP(e, hipFree(sl.d));
        sl.d = nullptr;
    }
    for (ChunkStage::Slot &sl : c.slot) {
        BV_HIP(e, hipHostMalloc(reinterpret_cast<void **>(&sl.h), up256(bytes) + back_bytes));
        BV_HIP(e, hipMalloc(reinterpret_cast<void **>(&sl.d), bytes));
        sl.back = sl.h + up256(bytes);
    }
    c.cap = bytes; c.back_cap = back_bytes;
    return BV_OK;
}

// host: the pinned chunk of slot s has crossed the link and may be written
inline int chunk_stage_fill(bv_engine *e, ChunkStage &c, unsigned s) {
    if (c.slot[s].used) BV_HIP(e, hipEventSynchronize(c.slot[s].copied));
    return BV_OK;
}

// The first `bytes` of slot s to the device, on `cs` and behind the last reader of the device chunk; `st` waits for them.
inline int chunk_stage_upload(bv_engine *e, ChunkStage &c, unsigned s, size_t bytes, hipStream_t st) {
    ChunkStage::Slot &sl = c.slot[s];
    if (bytes > c.cap) return fail(e, BV_ERR_INVALID_ARG, "chunk_stage_upload: " + std::to_string(bytes) + " bytes into chunks of " + std::to_string(c.cap));
    if (sl.used) BV_HIP(e, hipStreamWaitEvent(c.cs, sl.done, 0));
    BV_HIP(e, hipMemcpyAsync(sl.d, sl.h, bytes, hipMemcpyHostToDevice, c.cs));
    BV_HIP(e, hipEventRecord(sl.copied, c.cs));
    BV_HIP(e, hipStreamWaitEvent(st, sl.copied, 0));
    return BV_OK;
}

// what `st` holds now is the last reader of slot s (and the last writer of its `back`)
inline int chunk_stage_done(bv_engine *e, ChunkStage &c, unsigned s, hipStream_t st) {
    BV_HIP(e, hipEventRecord(c.slot[s].done, st));
    c.slot[s].used = true;
    return BV_OK;
}

// host: the kernels of slot s and the copies behind them are through
inline int chunk_stage_wait_done(bv_engine *e, ChunkStage &c, unsigned s) {
    BV_HIP(e, hipEventSynchronize(c.slot[s].done));
    return BV_OK;
}

// (the owner has selected the device)
inline void chunk_stage_free(ChunkStage &c) {
    if (c.cs) (void)hipStreamSynchronize(c.cs);
    for (ChunkStage::Slot &sl : c.slot) {
        if (sl.h) (void)hipHostFree(sl.h);
        if (sl.d) (void)hipFree(sl.d);
        if (sl.copied) (void)hipEventDestroy(sl.copied);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    if (c.cs) (void)hipStreamDestroy(c.cs);
    c = ChunkStage();
}

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// A smaller chunk from the environment, for tests of the staging's reuse: never above `dflt`; unset, 0 or no number -> `dflt`.
inline size_t chunk_limit_from_env(const char *name, size_t dflt) {
    if (const char *v = std::getenv(name)) {
        const unsigned long long x = std::strtoull(v, nullptr, 10);
        if (x > 0 && x < dflt) return (size_t)x;
    }
    return dflt;
}

// A kernel whose static LDS is more than the 64 KiB every launch may have: does this device take it?  Asked once (*fits).
// `who`: "<entry point>: the <...> kernel", for the message.
inline int kernel_lds_fits(bv_engine *e, const char *who, const void *kernel, int device, bool *fits) {
    if (*fits) return BV_OK;
    hipFuncAttributes fa;
    BV_HIP(e, hipFuncGetAttributes(&fa, kernel));
    int lds_max = 0;
    BV_HIP(e, hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    if (fa.sharedSizeBytes > (size_t)lds_max)
        return fail(e, BV_ERR_NO_DEVICE, std::string(who) + " needs " + std::to_string(fa.sharedSizeBytes) +
                                             " bytes of LDS per workgroup, the device offers " + std::to_string(lds_max));
    *fits = true;
    return BV_OK;
}

}  // namespace bv_impl
