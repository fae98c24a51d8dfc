// bv_indel_tally.hip -- the CVG rows' indel columns tallied on the device from the rows' indel tokens (bv_engine_indel_tally,
// bv_engine_indel_fetch; include/basevar_amd_indel.h; the contract is INTEGRATION.md section 2m).  The bytes and the domain are
// defined at the head of bv_indel_tally_core.h, which a CPU harness compiles too; this file is their schedule.
//
// The tokens ascend by pos, so a row's tokens are one range of them: every wave finds its row's by two binary searches for the
// row's key (a row without tokens ends there) and tallies it class first -- realistic rows carry many tokens of few classes:
//   keys     lane l takes tokens l, 64 + l, ...: bounds of the text checked, then the token's key and filter state into LDS
//   classes  the first token of no class is the representative; all lanes compare theirs with it in steps of 64 (keys first, the
//            text only behind equal keys and lengths), mark the equal ones and count them; until no token is left.  A lane only
//            ever reads the class marks it wrote itself.  The running sum of the entries ends a row that leaves the domain.
//   ranks    lane l takes classes l, 64 + l, ...: bv_it_class_at over the representatives, the one ranking routine
//   count    the column's length is the greatest entry end; the lengths and the flags are summed and decided on the HOST, which
//            waits for the counts to size the text anyway
//   write    classes and ranks again, by the same two device functions; a lane stores its class's entry, the text of a long one
//            is stored by the whole wave.  Every byte of a column has one writer.
// Device tokens are checked by a kernel of their own before (pos ascending, the text inside text_bytes): its per-block counts
// are summed on the host.  No atomics, no scratch, vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/basevar_amd_indel.h"
#include "bv_chunk_stage.h"
#include "bv_device_text.h"
#include "bv_indel_tally_core.h"
#include "bv_pileup_core.h"
#include "bv_text_image.h"

using namespace bv_impl;

static_assert(sizeof(bv_it_token) == sizeof(bv_pileup_token) && sizeof(bv_it_token) == sizeof(BvPileupToken) && sizeof(bv_it_token) == 24, "one token layout");
static_assert(BV_IT_COLUMN_MAX == BV_RECORD_TEXT_INDEL_MAX, "the core restates the record text's bound");
static_assert(BV_INDEL_ROW_TOKENS_MAX < BV_IT_DROPPED && BV_IT_COLUMN_MAX + 1u <= 0xffffu, "class numbers and entry offsets are 16 bits wide");

namespace {

constexpr uint32_t kMaxTok = BV_INDEL_ROW_TOKENS_MAX;
constexpr uint32_t kWaveText = 32u;       // an entry's text of more bytes is stored by the whole wave
constexpr uint32_t kCheckPerLane = 16u;   // tokens a lane of the check kernel looks at

struct ItArgs {
    const bv_it_token *tok;   // [n_tokens] ascending by pos
    const uint8_t *text;
    const uint32_t *key;      // [n]
    uint64_t n_tokens, text_bytes;
    uint32_t *len, *flag;     // count: [n]
    uint8_t *out;             // write
    const uint64_t *col_off;  // write: [n + 1]
    uint32_t n;
    uint32_t cap;             // tokens of a row the launch's LDS holds: a multiple of 64, at most kMaxTok
};

// The working storage of one row, carved from the launch's dynamic LDS: keys and class marks for `cap` tokens (the launch's
// longest row, in whole steps), class tables for the classes that many tokens, or a column inside the domain, can make
struct RowLds {
    uint32_t *key;
    uint16_t *cls, *rep, *cnt, *at;
};

__host__ __device__ inline uint32_t classes_of(uint32_t cap) { return cap < BV_IT_CLASSES_MAX ? cap : BV_IT_CLASSES_MAX; }
__host__ __device__ inline uint32_t lds_bytes(uint32_t cap) { return 6u * cap + 6u * classes_of(cap); }  // (cap a multiple of 64: every part 16-byte aligned)

__device__ inline RowLds row_lds(uint8_t *lds, uint32_t cap) {
    RowLds s;
    s.key = reinterpret_cast<uint32_t *>(lds);
    s.cls = reinterpret_cast<uint16_t *>(lds + 4u * cap);
    s.rep = s.cls + cap;
    s.cnt = s.rep + classes_of(cap);
    s.at = s.cnt + classes_of(cap);
    return s;
}

// the first token whose pos is not below `key` (above: not below or equal), in [lo, n): wave-uniform
__device__ inline uint64_t first_not_below(const bv_it_token *tok, uint64_t lo, uint64_t n, uint32_t key, bool above) {
    uint64_t hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        const uint32_t p = tok[mid].pos;
        if (above ? p <= key : p < key) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// Row k's tokens as a bv_it_row over the LDS storage; false: it has none
__device__ inline bool row_of(const ItArgs &a, uint32_t k, const RowLds &s, bv_it_row *r, uint64_t *n_row) {
    const uint32_t key = a.key[k];
    const uint64_t lo = first_not_below(a.tok, 0, a.n_tokens, key, false), hi = first_not_below(a.tok, lo, a.n_tokens, key, true);
    *n_row = hi - lo;
    r->tok = a.tok + lo; r->text = a.text;
    r->n = (uint32_t)min(hi - lo, (uint64_t)a.cap);
    r->key = s.key; r->cls = s.cls; r->rep = s.rep; r->cnt = s.cnt;
    return hi != lo;
}

// bv_it_classify over the lanes; wave-uniform result
__device__ inline int classify(const bv_it_row &r, uint64_t n_row, uint64_t text_bytes, uint32_t lane, uint32_t *n_cls) {
    *n_cls = 0;
    if (n_row > r.n) return BV_IT_OUTSIDE;  // (more than the LDS holds: the host sized it for every row inside the domain)
    const uint32_t m = r.n;
    uint32_t bad = 0;
    for (uint32_t i = lane; i < m; i += 64u)
        if (!bv_it_token_prepare(&r, i, text_bytes)) bad = 1;
    if (wave_sum(bad)) return BV_IT_BAD;
    __syncthreads();  // a token's key is read by every lane once the token is a representative
    uint32_t sum = 0, c = 0, from = 0;
    for (;;) {
        uint32_t rep = m;
        for (uint32_t base = from; base < m; base += 64u) {
            const uint32_t i = base + lane;
            const uint64_t open = __ballot(i < m && r.cls[i] == BV_IT_UNASSIGNED);
            if (open) { rep = base + (uint32_t)__ffsll((unsigned long long)open) - 1u; break; }
            from = base + 64u;  // (no token of this step is left)
        }
        if (rep >= m) break;
        uint32_t count = 0;
        for (uint32_t base = rep & ~63u; base < m; base += 64u) {
            const uint32_t i = base + lane;
            if (i >= rep && i < m && r.cls[i] == BV_IT_UNASSIGNED && bv_it_same(&r, rep, i)) { r.cls[i] = (uint16_t)c; ++count; }
        }
        count = wave_sum(count);
        if (!bv_it_column_grow(&sum, r.tok[rep].text_len, count)) return BV_IT_OUTSIDE;  // (so c < BV_IT_CLASSES_MAX here)
        if (lane == 0) { r.rep[c] = (uint16_t)rep; r.cnt[c] = (uint16_t)count; }
        ++c;
    }
    __syncthreads();  // rep / cnt, written by lane 0, are read by every lane
    *n_cls = c;
    return BV_IT_OK;
}

// bv_it_class_at of every class into s.at; returns the column's length (wave-uniform)
__device__ inline uint32_t rank_classes(const bv_it_row &r, uint32_t n_cls, const RowLds &s, uint32_t lane) {
    uint32_t end = 0;
    for (uint32_t c = lane; c < n_cls; c += 64u) {
        const uint32_t at = bv_it_class_at(&r, n_cls, c);
        s.at[c] = (uint16_t)at;
        end = max(end, at + bv_it_entry_len(r.tok[r.rep[c]].text_len, r.cnt[c]));
    }
    for (int d = 32; d > 0; d >>= 1) end = max(end, (uint32_t)__shfl_xor(end, d, 64));
    return end;
}

extern __shared__ __attribute__((aligned(16))) uint8_t bv_it_lds[];

__global__ __launch_bounds__(64) void bv_it_count_kernel(ItArgs a) {
    const RowLds s = row_lds(bv_it_lds, a.cap);
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= a.n) return;
    bv_it_row r;
    uint64_t n_row;
    uint32_t len = 0, flag = BV_IT_OK, n_cls = 0;
    if (row_of(a, k, s, &r, &n_row)) {
        flag = (uint32_t)classify(r, n_row, a.text_bytes, lane, &n_cls);
        if (flag == BV_IT_OK) len = rank_classes(r, n_cls, s, lane);
        if (flag == BV_IT_OK && len > BV_IT_COLUMN_MAX) { flag = BV_IT_OUTSIDE; len = 0; }
    }
    if (lane == 0) { a.len[k] = len; a.flag[k] = flag; }
}

__global__ __launch_bounds__(64) void bv_it_write_kernel(ItArgs a) {
    const RowLds s = row_lds(bv_it_lds, a.cap);
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= a.n) return;
    const uint64_t dst = a.col_off[k], bytes = a.col_off[k + 1u] - dst;
    if (bytes == 0 || bytes > BV_IT_COLUMN_MAX) return;
    bv_it_row r;
    uint64_t n_row;
    uint32_t n_cls = 0;
    if (!row_of(a, k, s, &r, &n_row) || classify(r, n_row, a.text_bytes, lane, &n_cls) != BV_IT_OK) return;
    // (the tokens are the count kernel's, so the column is `bytes` long; were they not, nothing is stored beyond the column)
    if (rank_classes(r, n_cls, s, lane) != (uint32_t)bytes) return;
    __syncthreads();
    uint8_t *out = a.out + dst;
    const uint32_t total = (uint32_t)bytes;
    for (uint32_t base = 0; base < n_cls; base += 64u) {
        const uint32_t c = base + lane;
        uint32_t len = 0;
        if (c < n_cls) {
            const uint32_t i = r.rep[c], at = s.at[c];
            len = r.tok[i].text_len;
            if (len <= kWaveText) {
                const uint8_t *t = bv_it_text(&r, i);
                for (uint32_t j = 0; j < len; ++j) out[at + j] = t[j];
            }
            bv_it_entry_tail_put(r.cnt[c], at + bv_it_entry_len(len, r.cnt[c]) == total, out + at + len);
        }
        for (uint64_t wide = __ballot(len > kWaveText); wide; wide &= wide - 1u) {
            const uint32_t cw = base + (uint32_t)__ffsll((unsigned long long)wide) - 1u, i = r.rep[cw], n = r.tok[i].text_len;
            const uint8_t *t = bv_it_text(&r, i);
            uint8_t *o = out + s.at[cw];
            for (uint32_t j = lane; j < n; j += 64u) o[j] = t[j];
        }
    }
}

// Tokens as a caller left them in device memory: per block, how many descend against their predecessor or leave the text
__global__ __launch_bounds__(64) void bv_it_check_kernel(const bv_it_token *tok, uint64_t n_tokens, uint64_t text_bytes, uint32_t *bad_of_block) {
    const uint32_t lane = threadIdx.x;
    const uint64_t first = ((uint64_t)blockIdx.x * 64u + lane) * kCheckPerLane;
    uint32_t bad = 0;
    for (uint64_t i = first; i < first + kCheckPerLane && i < n_tokens; ++i) {
        if (!bv_it_token_ok(tok + i, text_bytes)) ++bad;
        if (i && tok[i].pos < tok[i - 1u].pos) ++bad;
    }
    bad = wave_sum(bad);
    if (lane == 0) bad_of_block[blockIdx.x] = bad;
}

}  // namespace

// Per-engine state: the columns of the last tally, and what the kernels read and leave
struct BvIndelState {
    DeviceText text;
    uint8_t *d_in = nullptr;    // uploaded tokens and their text, the keys
    uint8_t *d_out = nullptr;   // len u32 [n], flag u32 [n]; the check kernel's counts
    uint8_t *d_off = nullptr;   // col_off u64 [n + 1] of the last tally
    size_t in_cap = 0, out_cap = 0, off_cap = 0;
    uint32_t n = 0;
    std::vector<uint8_t> flag;  // [n] of the last tally
};

void bv_indel_state_free(BvIndelState *t) {
    if (!t) return;
    (void)hipSetDevice(t->text.device);
    for (uint8_t *b : {t->text.d_text, t->d_in, t->d_out, t->d_off})
        if (b) (void)hipFree(b);
    delete t;
}

void bv_indel_view(const BvIndelState *t, BvIndelView *v) {
    *v = BvIndelView();
    if (!t || !t->text.formatted) return;
    v->done = true; v->n = t->n;
    v->d_text = t->text.d_text; v->d_off = reinterpret_cast<const uint64_t *>(t->d_off); v->flag = t->flag.data();
}

extern "C" {

uint32_t bv_indel_row_tokens_max(void) { return BV_INDEL_ROW_TOKENS_MAX; }

int bv_engine_indel_tally(bv_engine *e, const bv_indel_tokens *tok, const uint32_t *key, uint32_t n, uint64_t *col_off, uint8_t *row_flag, void *stream_) {
    const std::string who = "bv_engine_indel_tally: ";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    if (!col_off || (n && (!key || !row_flag))) return fail(e, BV_ERR_INVALID_ARG, who + "null key/col_off/row_flag");
    if (n >= (1u << 26)) return fail(e, BV_ERR_TOO_LARGE, who + "2^26 rows or more: tally fewer rows a call");
    const bv_it_token *h_tok = nullptr;  // descriptors to upload
    const uint8_t *text = nullptr;
    uint64_t n_tokens = 0, text_bytes = 0;
    bool up_tok = true, up_text = false, check_on_device = false;
    if (!tok) {
        BvPileupView v;
        bv_pileup_view(e->pileup, &v);
        if (!e->pileup || !v.done) return fail(e, BV_ERR_INVALID_ARG, who + "tok == NULL, and no completed bv_engine_pileup on this engine");
        h_tok = reinterpret_cast<const bv_it_token *>(v.tokens);
        n_tokens = v.n_tokens; text = v.d_text; text_bytes = v.text_bytes;
    } else {
        if (tok->reserved_) return fail(e, BV_ERR_INVALID_ARG, who + "reserved_ must be zero");
        if (tok->mem_kind != BV_MEM_HOST && tok->mem_kind != BV_MEM_DEVICE) return fail(e, BV_ERR_INVALID_ARG, who + "mem_kind must be BV_MEM_HOST or BV_MEM_DEVICE");
        if ((tok->n_tokens && !tok->tokens) || (tok->text_bytes && !tok->text)) return fail(e, BV_ERR_INVALID_ARG, who + "null tokens/text");
        n_tokens = tok->n_tokens; text = tok->text; text_bytes = tok->text_bytes;
        if (tok->mem_kind == BV_MEM_HOST) {
            h_tok = reinterpret_cast<const bv_it_token *>(tok->tokens);
            up_text = true;
            for (uint64_t i = 0; i < n_tokens; ++i) {
                if (i && h_tok[i].pos < h_tok[i - 1].pos) return fail(e, BV_ERR_INVALID_ARG, who + "token " + std::to_string(i) + ": pos descends");
                if (!bv_it_token_ok(h_tok + i, text_bytes)) return fail(e, BV_ERR_INVALID_ARG, who + "token " + std::to_string(i) + " runs beyond text_bytes");
            }
        } else {
            up_tok = false;
            check_on_device = n_tokens != 0;
        }
    }
    BvIndelState *t = text_state(e, e->indel);
    if (n == 0) {
        t->n = 0; t->flag.clear();
        return device_text_empty(t->text, col_off);
    }
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    BV_HIP(e, hipSetDevice(t->text.device));
    const uint32_t n_check = check_on_device ? (uint32_t)std::min<uint64_t>((n_tokens + 64u * kCheckPerLane - 1u) / (64u * kCheckPerLane), 0x7fffffffu) : 0u;
    if (check_on_device && (n_tokens + 64u * kCheckPerLane - 1u) / (64u * kCheckPerLane) > n_check) return fail(e, BV_ERR_TOO_LARGE, who + "2^41 tokens or more");
    size_t at = 0;
    auto place = [&at](size_t bytes) { const size_t o = at; at += up16(bytes); return o; };
    const size_t o_key = place(4ull * n), o_tok = place(up_tok ? sizeof(bv_it_token) * n_tokens : 0), o_text = place(up_text ? text_bytes : 0);
    int rc = grow_device(e, &t->d_in, &t->in_cap, at + 16);
    if (rc == BV_OK) rc = grow_device(e, &t->d_out, &t->out_cap, 8ull * n + 4ull * n_check + 16);
    if (rc != BV_OK) return rc;
    BV_HIP(e, hipMemcpyAsync(t->d_in + o_key, key, 4ull * n, hipMemcpyHostToDevice, st));
    if (up_tok && n_tokens) BV_HIP(e, hipMemcpyAsync(t->d_in + o_tok, h_tok, sizeof(bv_it_token) * n_tokens, hipMemcpyHostToDevice, st));
    if (up_text && text_bytes) BV_HIP(e, hipMemcpyAsync(t->d_in + o_text, text, text_bytes, hipMemcpyHostToDevice, st));
    ItArgs a;
    a.tok = up_tok ? reinterpret_cast<const bv_it_token *>(t->d_in + o_tok) : reinterpret_cast<const bv_it_token *>(tok->tokens);
    a.text = up_text ? t->d_in + o_text : text;
    a.key = reinterpret_cast<const uint32_t *>(t->d_in + o_key);
    a.n_tokens = n_tokens; a.text_bytes = text_bytes;
    a.len = reinterpret_cast<uint32_t *>(t->d_out); a.flag = a.len + n;
    a.out = nullptr; a.col_off = nullptr; a.n = n;
    // the LDS a wave gets: for the launch's longest row where the host has the descriptors, for the domain's where it has not
    uint64_t longest = kMaxTok;
    if (up_tok) {
        longest = 1;
        auto below = [](const bv_it_token &x, uint32_t p) { return x.pos < p; };
        auto above = [](uint32_t p, const bv_it_token &x) { return p < x.pos; };
        for (uint32_t k = 0; k < n; ++k) {
            const bv_it_token *lo = std::lower_bound(h_tok, h_tok + n_tokens, key[k], below);
            longest = std::max<uint64_t>(longest, (uint64_t)(std::upper_bound(lo, h_tok + n_tokens, key[k], above) - lo));
        }
    }
    a.cap = (uint32_t)((std::min<uint64_t>(longest, kMaxTok) + 63u) / 64u * 64u);
    const uint32_t lds = lds_bytes(a.cap);
    if (lds > 48u * 1024u) {
        BV_HIP(e, hipFuncSetAttribute(reinterpret_cast<const void *>(bv_it_count_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        BV_HIP(e, hipFuncSetAttribute(reinterpret_cast<const void *>(bv_it_write_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    uint32_t *d_check = a.flag + n;
    if (n_check) {
        hipLaunchKernelGGL(bv_it_check_kernel, dim3(n_check), dim3(64), 0, st, a.tok, n_tokens, text_bytes, d_check);
        BV_HIP(e, hipGetLastError());
    }
    hipLaunchKernelGGL(bv_it_count_kernel, dim3(n), dim3(64), lds, st, a);
    BV_HIP(e, hipGetLastError());
    std::vector<uint32_t> back(2ull * n + n_check);
    BV_HIP(e, hipMemcpyAsync(back.data(), t->d_out, 4ull * back.size(), hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    for (uint32_t b = 0; b < n_check; ++b)
        if (back[2ull * n + b])
            return fail(e, BV_ERR_INVALID_ARG, who + "device tokens " + std::to_string((uint64_t)b * 64u * kCheckPerLane) + " ..: a pos descends, or a token runs beyond text_bytes");
    for (uint32_t k = 0; k < n; ++k)
        if (back[n + k] == BV_IT_BAD) return fail(e, BV_ERR_INVALID_ARG, who + "row " + std::to_string(k) + ": a token runs beyond text_bytes");
    // from here on the last tally is replaced
    t->text.formatted = false;
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t k = 0; k < n; ++k) off[k + 1] = off[k] + back[k];
    rc = device_text_reserve(e, t->text, off[n]);
    if (rc == BV_OK) rc = grow_device(e, &t->d_off, &t->off_cap, 8ull * (n + 1));
    if (rc != BV_OK) return rc;
    BV_HIP(e, hipMemcpyAsync(t->d_off, off.data(), 8ull * (n + 1), hipMemcpyHostToDevice, st));
    if (off[n]) {
        a.out = t->text.d_text; a.col_off = reinterpret_cast<const uint64_t *>(t->d_off);
        hipLaunchKernelGGL(bv_it_write_kernel, dim3(n), dim3(64), lds, st, a);
        BV_HIP(e, hipGetLastError());
    }
    BV_HIP(e, hipStreamSynchronize(st));
    t->n = n;
    t->flag.resize(n);
    for (uint32_t k = 0; k < n; ++k) t->flag[k] = row_flag[k] = (uint8_t)back[n + k];
    std::memcpy(col_off, off.data(), 8ull * (n + 1));
    device_text_done(t->text, off[n]);
    return BV_OK;
}

int bv_engine_indel_fetch(bv_engine *e, void *dst, uint64_t dst_capacity, int dst_mem_kind, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_indel_fetch: null engine");
    return device_text_fetch(e, "bv_engine_indel_fetch: ", "bv_engine_indel_tally", e->indel ? &e->indel->text : nullptr, dst, dst_capacity, dst_mem_kind, stream_);
}

}  // extern "C"
