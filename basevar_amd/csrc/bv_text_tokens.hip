// bv_text_tokens.hip -- the '+SEQ' / '-SEQ' tokens of parsed batchfile rows, taken on the device
// (include/basevar_amd_text_tokens.h; the contract is INTEGRATION.md section 2n, the result is defined at the head of
// bv_text_tokens_core.h).
//
// bv_text_parse_kernel only marks a row that holds such a token (BV_TEXT_INDEL).  With the mode on, the rows of a staged chunk
// (bv_engine_text_parse) or of the whole inflated text (bv_engine_text_parse_bgzf) go through count, scan and write while
// their text is on the device: one wave per row, an unmarked row leaves at once; a marked row is walked 64 bytes a step with
// the parser's ballots, and the masks of bv_text_tokens_core.h say which lane holds token text, a token's first byte or the
// separator that ends it.  The scan gives every row its place in the descriptors and in the text, running on from chunk to
// chunk; the host waits once per chunk for the two sums and grows the store.  After the parse has fixed the positions' final
// states, the rows of positions in state 0 are packed into the list the caller gets: descriptors and text without gaps.
// No atomics, no LDS in the walk, vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/basevar_amd_text_tokens.h"
#include "bv_engine_impl.h"
#include "bv_text_tokens_core.h"
#include "bv_text_tokens_walk.h"

using namespace bv_impl;

static_assert(sizeof(bv_tt_token) == sizeof(bv_pileup_token) && sizeof(bv_tt_token) == 24, "bv_tt_token is bv_pileup_token");

namespace {

// One wave per row of the chunk; four rows per workgroup.
__global__ __launch_bounds__(256) void bv_tt_count_kernel(TokArgs a) {
    const uint32_t local = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (local >= a.n_rows) return;
    walk_row<false>(a, a.row_first + local, a.row_first + local, threadIdx.x & 63u);
}
__global__ __launch_bounds__(256) void bv_tt_write_kernel(TokArgs a) {
    const uint32_t local = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (local >= a.n_rows) return;
    walk_row<true>(a, a.row_first + local, a.row_first + local, threadIdx.x & 63u);
}

// Rows [first, first + n) scanned (scan_rows of bv_text_tokens_walk.h).  One workgroup.
__global__ __launch_bounds__(kScanThreads) void bv_tt_scan_kernel(const uint32_t *ca, const uint32_t *cb, const uint8_t *pos_state, uint32_t F, uint32_t first,
                                                                  uint32_t n, uint64_t start_a, uint64_t start_b, uint64_t *out_a, uint64_t *out_b,
                                                                  uint64_t *totals) {
    scan_rows<false>(ca, cb, pos_state, F, first, n, start_a, start_b, out_a, out_b, totals, 0u, 0u);
}
// The rows of positions in state 0 into the caller's list: one wave per row moves its descriptors and its text.
struct PackArgs {
    const uint32_t *cnt_tok, *cnt_txt;
    const uint64_t *base_tok, *base_txt, *to_tok, *to_txt;
    const uint8_t *pos_state;
    const bv_tt_token *tok;
    const uint8_t *ttext;
    bv_tt_token *out_tok;
    uint8_t *out_text;
    uint32_t n_rows, n_files;
};
__global__ __launch_bounds__(256) void bv_tt_pack_kernel(PackArgs a) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (r >= a.n_rows) return;
    const uint32_t nt = a.cnt_tok[r], nx = a.cnt_txt[r];
    if (nt == 0 || a.pos_state[r / a.n_files] != 0) return;
    const uint64_t from_txt = a.base_txt[r], to_txt = a.to_txt[r];
    const bv_tt_token *src = a.tok + a.base_tok[r];
    bv_tt_token *dst = a.out_tok + a.to_tok[r];
    for (uint32_t i = lane; i < nt; i += 64u) {
        bv_tt_token t = src[i];
        t.text_off = t.text_off - from_txt + to_txt;
        dst[i] = t;
    }
    for (uint32_t i = lane; i < nx; i += 64u) a.out_text[to_txt + i] = a.ttext[from_txt + i];
}

}  // namespace

// Per-engine state: the mode, the store that the chunks fill, and the list of the last parse.
struct BvTextTokState {
    int device = 0;
    bool on = false;
    bool valid = false;             // the list of the engine's last parse stands
    uint8_t *d_rows = nullptr;      // cnt_tok, cnt_txt u32 [R]; base_tok, base_txt, to_tok, to_txt u64 [R]; totals u64 [2]; pos_state [P]
    size_t rows_bytes = 0;
    uint8_t *d_tok = nullptr, *d_ttext = nullptr;  // the store: descriptors and text of every marked row, in row order
    size_t tok_bytes = 0, ttext_bytes = 0;
    uint8_t *d_list = nullptr, *d_ltext = nullptr; // the list: the store's rows of positions in state 0
    size_t list_bytes = 0, ltext_bytes = 0;
    uint32_t n_rows = 0;            // R of the parse under way
    uint64_t run_tok = 0, run_txt = 0;     // the store's fill
    uint64_t n_tokens = 0, text_bytes = 0; // the list
    uint32_t *cnt_tok() const { return reinterpret_cast<uint32_t *>(d_rows); }
    uint32_t *cnt_txt() const { return cnt_tok() + n_rows; }
    uint64_t *u64(unsigned k) const { return reinterpret_cast<uint64_t *>(d_rows + up256(8ull * n_rows) * (k + 1u)); }  // k: 0 base_tok .. 3 to_txt, 4 totals
    uint8_t *pos_state() const { return d_rows + up256(8ull * n_rows) * 5u + 256u; }
};

void bv_text_tok_state_free(BvTextTokState *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    for (uint8_t *b : {t->d_rows, t->d_tok, t->d_ttext, t->d_list, t->d_ltext})
        if (b) (void)hipFree(b);
    delete t;
}

namespace {
// A store that grows and keeps its first `used` bytes.
int grow_keep(bv_engine *e, uint8_t **buf, size_t *bytes, size_t need, size_t used, hipStream_t st) {
    if (need <= *bytes) return BV_OK;
    const size_t want = std::max(need, 2 * *bytes);
    uint8_t *nb = nullptr;
    BV_HIP(e, hipMalloc(reinterpret_cast<void **>(&nb), want));
    if (used) {
        hipError_t s = hipMemcpyAsync(nb, *buf, used, hipMemcpyDeviceToDevice, st);
        if (s == hipSuccess) s = hipStreamSynchronize(st);
        if (s != hipSuccess) {
            (void)hipFree(nb);
            return fail(e, BV_ERR_HIP, std::string("bv_text_tokens: moving the token store: ") + hipGetErrorString(s));
        }
    }
    uint8_t *old = *buf;
    *buf = nb; *bytes = want;  // (first: a failing hipFree leaves the store in the new buffer, nothing dangling and nothing leaked but `old`)
    if (old) BV_HIP(e, hipFree(old));
    return BV_OK;
}
}  // namespace

namespace bv_impl {

bool bv_text_tokens_stand(const bv_engine *e) { return e->ttok && e->ttok->on && e->ttok->valid; }
bool bv_text_tokens_on(const bv_engine *e) { return e->ttok && e->ttok->on; }

int bv_text_tokens_begin(bv_engine *e, uint32_t P, uint32_t F, hipStream_t st) {
    BvTextTokState *t = e->ttok;
    if (!t) return BV_OK;
    t->valid = false;
    if (!t->on) return BV_OK;
    (void)st;
    const size_t R = (size_t)P * F;
    t->n_rows = (uint32_t)R;
    t->run_tok = t->run_txt = 0;
    t->n_tokens = t->text_bytes = 0;
    return grow_device(e, &t->d_rows, &t->rows_bytes, up256(8ull * R) * 5u + 256u + up256(P));
}

int bv_text_tokens_rows(bv_engine *e, const BvTextTokRows &rows, hipStream_t st) {
    BvTextTokState *t = e->ttok;
    if (!t || !t->on || rows.n_rows == 0) return BV_OK;
    const bool job = rows.add_files != 0;  // the rows of a parse job's add: row_first and n_rows count the add's rows
    const uint64_t last = (uint64_t)rows.row_first + rows.n_rows - 1u;  // the last row, and with a job its place in the batch
    if (job && (uint64_t)rows.first_file + rows.add_files > rows.n_files) return fail(e, BV_ERR_INVALID_ARG, "bv_text_tokens_rows: files beyond the batch");
    if ((job ? last / rows.add_files * rows.n_files + rows.first_file + last % rows.add_files : last) >= t->n_rows)
        return fail(e, BV_ERR_INVALID_ARG, "bv_text_tokens_rows: rows beyond the batch");
    TokArgs a;
    a.text = rows.text; a.row_beg = rows.row_beg; a.row_end = rows.row_end; a.rowflag = rows.rowflag; a.foff = rows.foff;
    a.chunk_base = rows.chunk_base; a.row_first = rows.row_first; a.n_rows = rows.n_rows; a.n_files = rows.n_files;
    a.cnt_tok = t->cnt_tok(); a.cnt_txt = t->cnt_txt(); a.base_tok = t->u64(0); a.base_txt = t->u64(1);
    a.tok = nullptr; a.ttext = nullptr;
    const dim3 grid((rows.n_rows + 3u) / 4u);
    BvTextTokStore store{t->cnt_tok(), t->cnt_txt(), t->u64(0), t->u64(1), t->u64(4), nullptr, nullptr};
    if (job) {  // (the strided kernels live with the job: bv_text_job.hip)
        text_job_tokens_count_scan(rows, store, t->run_tok, t->run_txt, st);
    } else {
        hipLaunchKernelGGL(bv_tt_count_kernel, grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL(bv_tt_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t *)a.cnt_tok, (const uint32_t *)a.cnt_txt,
                           (const uint8_t *)nullptr, rows.n_files, rows.row_first, rows.n_rows, t->run_tok, t->run_txt, t->u64(0), t->u64(1), t->u64(4));
    }
    BV_HIP(e, hipGetLastError());
    uint64_t sums[2] = {0, 0};
    BV_HIP(e, hipMemcpyAsync(sums, t->u64(4), 16, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    if (sums[0] == t->run_tok) return BV_OK;  // no token in these rows
    int rc = grow_keep(e, &t->d_tok, &t->tok_bytes, sizeof(bv_tt_token) * sums[0], sizeof(bv_tt_token) * t->run_tok, st);
    if (rc == BV_OK) rc = grow_keep(e, &t->d_ttext, &t->ttext_bytes, sums[1], t->run_txt, st);
    if (rc != BV_OK) return rc;
    a.tok = reinterpret_cast<bv_tt_token *>(t->d_tok); a.ttext = t->d_ttext;
    store.tok = t->d_tok; store.ttext = t->d_ttext;
    if (job) text_job_tokens_write(rows, store, st);
    else hipLaunchKernelGGL(bv_tt_write_kernel, grid, dim3(256), 0, st, a);
    BV_HIP(e, hipGetLastError());
    t->run_tok = sums[0]; t->run_txt = sums[1];
    return BV_OK;
}

int bv_text_tokens_finish(bv_engine *e, const uint8_t *pos_state, uint32_t P, uint32_t F, hipStream_t st) {
    BvTextTokState *t = e->ttok;
    if (!t || !t->on) return BV_OK;
    const uint32_t R = t->n_rows;
    if ((uint64_t)P * F != R) return fail(e, BV_ERR_INVALID_ARG, "bv_text_tokens_finish: not the batch that was begun");
    if (t->run_tok) {
        BV_HIP(e, hipMemcpyAsync(t->pos_state(), pos_state, P, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(bv_tt_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t *)t->cnt_tok(), (const uint32_t *)t->cnt_txt(),
                           (const uint8_t *)t->pos_state(), F, 0u, R, (uint64_t)0, (uint64_t)0, t->u64(2), t->u64(3), t->u64(4));
        BV_HIP(e, hipGetLastError());
        uint64_t sums[2] = {0, 0};
        BV_HIP(e, hipMemcpyAsync(sums, t->u64(4), 16, hipMemcpyDeviceToHost, st));
        BV_HIP(e, hipStreamSynchronize(st));
        if (sums[0] > t->run_tok || sums[1] > t->run_txt) return fail(e, BV_ERR_HIP, "bv_text_tokens_finish: the list is larger than the store");
        if (sums[0]) {
            int rc = grow_device(e, &t->d_list, &t->list_bytes, sizeof(bv_tt_token) * sums[0]);
            if (rc == BV_OK) rc = grow_device(e, &t->d_ltext, &t->ltext_bytes, sums[1]);
            if (rc != BV_OK) return rc;
            PackArgs a;
            a.cnt_tok = t->cnt_tok(); a.cnt_txt = t->cnt_txt(); a.base_tok = t->u64(0); a.base_txt = t->u64(1); a.to_tok = t->u64(2); a.to_txt = t->u64(3);
            a.pos_state = t->pos_state(); a.tok = reinterpret_cast<const bv_tt_token *>(t->d_tok); a.ttext = t->d_ttext;
            a.out_tok = reinterpret_cast<bv_tt_token *>(t->d_list); a.out_text = t->d_ltext; a.n_rows = R; a.n_files = F;
            hipLaunchKernelGGL(bv_tt_pack_kernel, dim3((R + 3u) / 4u), dim3(256), 0, st, a);
            BV_HIP(e, hipGetLastError());
            BV_HIP(e, hipStreamSynchronize(st));
        }
        t->n_tokens = sums[0]; t->text_bytes = sums[1];
    }
    t->valid = true;
    return BV_OK;
}

}  // namespace bv_impl

extern "C" {

int bv_engine_text_tokens_enable(bv_engine *e, int on) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_text_tokens_enable: null engine");
    if (!on && !e->ttok) return BV_OK;
    engine_state(e, e->ttok)->on = on != 0;
    return BV_OK;
}

int bv_engine_text_tokens(bv_engine *e, bv_indel_tokens *out) {
    const char *who = "bv_engine_text_tokens";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, std::string(who) + ": null engine");
    if (!out) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null out");
    const BvTextTokState *t = e->ttok;
    if (!t || !t->on) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": the mode is off (bv_engine_text_tokens_enable)");
    if (!t->valid) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": no completed parse with the mode on");
    out->tokens = t->n_tokens ? reinterpret_cast<const bv_pileup_token *>(t->d_list) : nullptr;
    out->text = t->text_bytes ? t->d_ltext : nullptr;
    out->n_tokens = t->n_tokens; out->text_bytes = t->text_bytes;
    out->mem_kind = BV_MEM_DEVICE; out->reserved_ = 0;
    return BV_OK;
}

int bv_engine_text_tokens_fetch(bv_engine *e, bv_pileup_token *tokens, uint64_t tokens_capacity, uint8_t *text, uint64_t text_capacity, uint64_t *n_tokens,
                                uint64_t *text_bytes, void *stream_) {
    const char *who = "bv_engine_text_tokens_fetch";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, std::string(who) + ": null engine");
    if (!n_tokens || !text_bytes) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null n_tokens/text_bytes");
    const BvTextTokState *t = e->ttok;
    if (!t || !t->on) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": the mode is off (bv_engine_text_tokens_enable)");
    if (!t->valid) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": no completed parse with the mode on");
    *n_tokens = t->n_tokens; *text_bytes = t->text_bytes;
    if (tokens_capacity < t->n_tokens || text_capacity < t->text_bytes)
        return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": room for " + std::to_string(t->n_tokens) + " tokens and " + std::to_string(t->text_bytes) +
                                               " bytes of text is needed");
    if ((t->n_tokens && !tokens) || (t->text_bytes && !text)) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null tokens/text");
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    BV_HIP(e, hipSetDevice(t->device));
    if (t->n_tokens) BV_HIP(e, hipMemcpyAsync(tokens, t->d_list, sizeof(bv_pileup_token) * t->n_tokens, hipMemcpyDeviceToHost, st));
    if (t->text_bytes) BV_HIP(e, hipMemcpyAsync(text, t->d_ltext, t->text_bytes, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    return BV_OK;
}

}  // extern "C"
