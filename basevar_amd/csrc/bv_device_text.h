// bv_device_text.h -- a text that one of the engine's formatters left in device memory (bv_vcf.hip, bv_pileup_text.hip): its
// buffer, which the formatter's state holds as a member, and the fetch and the deflate call behind it are one piece of plumbing,
// stated here once.  Host-only.
#pragma once

#include <string>

#include "../../include/basevar_amd_bgzf.h"
#include "bv_engine_impl.h"

namespace bv_impl {

struct DeviceText {
    int device = 0;
    uint8_t *d_text = nullptr;  // the lines back to back, and room for the words a reader takes around them
    size_t cap = 0;
    uint64_t bytes = 0;
    bool formatted = false;     // d_text holds `bytes` bytes of a completed format call
};

// e->vcf, e->ptext: a formatter's state S, which holds its DeviceText as `text`, is created by the first call that needs it
template <class S>
S *text_state(bv_engine *e, S *&state) {
    if (!state) {
        state = new S();
        state->text.device = e->cfg.device;
    }
    return state;
}

// room for a text of `total` bytes, and 16 behind it: bv_deflate.hip's kernels read the whole aligned words around a block
inline int device_text_reserve(bv_engine *e, DeviceText &t, uint64_t total) { return grow_device(e, &t.d_text, &t.cap, up256(total + 16)); }

// the format call is complete: `total` bytes of text, which end at off[n]
inline void device_text_done(DeviceText &t, uint64_t total) {
    t.bytes = total;
    t.formatted = true;
}

// a format call of no lines: a completed text of no bytes, off[0] = 0
inline int device_text_empty(DeviceText &t, uint64_t *off) {
    off[0] = 0;
    device_text_done(t, 0);
    return BV_OK;
}

// `who`: "bv_engine_..._fetch: "; `format_call`: the call that must have come before; `t`: NULL before the first one
inline int device_text_fetch(bv_engine *e, const std::string &who, const char *format_call, const DeviceText *t, void *dst, uint64_t dst_capacity,
                             int dst_mem_kind, void *stream_) {
    if (!t || !t->formatted) return fail(e, BV_ERR_INVALID_ARG, who + "no " + format_call + " before it");
    if (dst_mem_kind != BV_MEM_HOST && dst_mem_kind != BV_MEM_DEVICE) return fail(e, BV_ERR_INVALID_ARG, who + "dst_mem_kind must be BV_MEM_HOST or BV_MEM_DEVICE");
    if (dst_capacity < t->bytes)
        return fail(e, BV_ERR_INVALID_ARG, who + "dst_capacity " + std::to_string(dst_capacity) + " < the text's " + std::to_string(t->bytes) + " bytes");
    if (t->bytes == 0) return BV_OK;
    if (!dst) return fail(e, BV_ERR_INVALID_ARG, who + "null dst");
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    BV_HIP(e, hipSetDevice(t->device));
    BV_HIP(e, hipMemcpyAsync(dst, t->d_text, t->bytes, dst_mem_kind == BV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    BV_HIP(e, hipStreamSynchronize(st));
    return BV_OK;
}

// the one encoder path: the formatted text is device text to bv_engine_bgzf_deflate_level, which checks the rest
inline int device_text_deflate(bv_engine *e, const std::string &who, const char *format_call, const DeviceText *t, const uint64_t *block_off,
                               uint32_t n_blocks, int level, uint8_t *dst, uint64_t dst_capacity, uint64_t *member_off, void *stream_) {
    if (!t || !t->formatted) return fail(e, BV_ERR_INVALID_ARG, who + "no " + format_call + " before it");
    return bv_engine_bgzf_deflate_level(e, t->d_text, t->bytes, BV_MEM_DEVICE, block_off, n_blocks, level, dst, dst_capacity, member_off, stream_);
}

}  // namespace bv_impl
