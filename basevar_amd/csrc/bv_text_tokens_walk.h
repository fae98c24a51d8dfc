// bv_text_tokens_walk.h -- the walk of one row for its '+SEQ' / '-SEQ' tokens and the scan of the rows' counts, as the kernels of
// bv_text_tokens.hip and the strided ones of a parse job's add (bv_text_job.hip) share them.  Device code; included by those two.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/basevar_amd_text_tokens.h"
#include "bv_text_tokens_core.h"

namespace {

struct TokArgs {
    const char *text;          // byte k is text byte chunk_base + k
    const uint64_t *row_beg, *row_end;
    const uint8_t *rowflag;
    const uint32_t *foff;
    uint64_t chunk_base;
    uint32_t row_first, n_rows, n_files;
    uint32_t *cnt_tok, *cnt_txt;            // [rows of the batch]
    const uint64_t *base_tok, *base_txt;    // [rows of the batch] (the write pass)
    bv_tt_token *tok;
    uint8_t *ttext;
};

// One wave walks row r of the batch, whose begin and end stand at index l (l == r but in a parse job's add, which brings its
// own rows' offsets).  WRITE: the lanes store what the masks give them, below the row's counts (a row that counted n tokens
// and m bytes stores nothing at or beyond them, whatever it reads).
template <bool WRITE>
__device__ __forceinline__ void walk_row(const TokArgs &a, uint32_t r, uint32_t l, uint32_t lane) {
    if (!(a.rowflag[r] & BV_TEXT_INDEL)) {
        if (!WRITE && lane == 0) { a.cnt_tok[r] = 0; a.cnt_txt[r] = 0; }
        return;
    }
    const char *row = a.text + (a.row_beg[l] - a.chunk_base);
    const uint32_t len = (uint32_t)(a.row_end[l] - a.row_beg[l]);
    const uint32_t p = r / a.n_files, f = r - p * a.n_files;
    const uint32_t sample0 = a.foff[f];
    uint32_t lim_tok = 0, lim_txt = 0;
    uint64_t at_tok = 0, at_txt = 0;
    if (WRITE) { lim_tok = a.cnt_tok[r]; lim_txt = a.cnt_txt[r]; at_tok = a.base_tok[r]; at_txt = a.base_txt[r]; }
    bv_tt_carry c = bv_tt_carry_init();
    for (uint32_t b = 0; b < len && !bv_tt_done(c); b += 64u) {
        const uint32_t i = b + lane;
        const bool valid = i < len;
        const char ch = valid ? row[i] : '\0';
        const uint64_t T = __ballot(valid && ch == '\t');
        const uint64_t S = __ballot(valid && ch == ' ');
        const uint64_t SEP = T | S | __ballot(valid && ch == '\n');
        const uint64_t V = __ballot(valid);
        const uint64_t F5 = __ballot(bv_tt_field_at(c, T, lane) == BV_TT_FIELD);
        const uint64_t PM = __ballot(valid && (ch == '+' || ch == '-'));
        const bv_tt_masks m = bv_tt_step_masks(c, SEP, V, F5, PM);
        if (WRITE) {
            const uint64_t bit = 1ull << lane;
            if (m.M & bit) {
                const uint32_t x = bv_tt_text_at(c, m, lane);
                if (x < lim_txt) a.ttext[at_txt + x] = (uint8_t)ch;
                if (m.IS & bit) {
                    const uint32_t o = bv_tt_start_ord_at(c, m, lane);
                    if (o < lim_tok) {
                        bv_tt_token *t = a.tok + at_tok + o;
                        t->pos = p; t->sample = sample0 + bv_tt_tok_at(c, T, S, lane); t->text_off = at_txt + x; t->reserved_ = 0;
                    }
                }
            } else if (m.EN & bit) {
                const uint32_t o = bv_tt_end_ord_at(c, m, lane);
                if (o < lim_tok) a.tok[at_tok + o].text_len = bv_tt_end_len_at(c, m, lane);
            }
        }
        c = bv_tt_carry_next(c, m, T, S, SEP);
    }
    if (!WRITE && lane == 0) { a.cnt_tok[r] = c.n_tok; a.cnt_txt[r] = c.n_txt; }
}

// The rows of a parse job's add (include/basevar_amd_text_job.h): the add holds files [first_file, first_file + K) of the batch's
// n_files; its row l = p * K + k is row p * n_files + first_file + k of the batch.
__device__ __forceinline__ uint32_t job_row(uint32_t l, uint32_t n_files, uint32_t first_file, uint32_t K) {
    const uint32_t p = l / K;
    return p * n_files + first_file + (l - p * K);
}

// Rows [first, first + n): out_a[r] = start_a + the counts ca of the rows before r, out_b the same for cb; with pos_state, a
// row of a position not in state 0 counts nothing.  totals[0 .. 2) = the sums behind the last row.  One workgroup: every thread
// sums a run of rows, the runs' sums are scanned in LDS, and every thread walks its run again.
// JOB: the rows are [first, first + n) of a parse job's add of files [first_file, first_file + K), scanned in the add's order and
// written at their places in the batch.
constexpr uint32_t kScanThreads = 1024;
template <bool JOB>
__device__ __forceinline__ void scan_rows(const uint32_t *ca, const uint32_t *cb, const uint8_t *pos_state, uint32_t F, uint32_t first, uint32_t n,
                                          uint64_t start_a, uint64_t start_b, uint64_t *out_a, uint64_t *out_b, uint64_t *totals, uint32_t first_file,
                                          uint32_t K) {
    __shared__ uint64_t sa[kScanThreads], sb[kScanThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n + kScanThreads - 1u) / kScanThreads;
    const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
    uint64_t a = 0, b = 0;
    for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t r = JOB ? job_row(first + k, F, first_file, K) : first + k;
        const bool keep = !pos_state || pos_state[r / F] == 0;
        a += keep ? ca[r] : 0u;
        b += keep ? cb[r] : 0u;
    }
    sa[tid] = a; sb[tid] = b;
    __syncthreads();
    for (uint32_t o = 1; o < kScanThreads; o <<= 1) {
        const uint64_t va = tid >= o ? sa[tid - o] : 0u, vb = tid >= o ? sb[tid - o] : 0u;
        __syncthreads();
        sa[tid] += va; sb[tid] += vb;
        __syncthreads();
    }
    uint64_t ra = start_a + sa[tid] - a, rb = start_b + sb[tid] - b;
    for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t r = JOB ? job_row(first + k, F, first_file, K) : first + k;
        const bool keep = !pos_state || pos_state[r / F] == 0;
        out_a[r] = ra; out_b[r] = rb;
        ra += keep ? ca[r] : 0u;
        rb += keep ? cb[r] : 0u;
    }
    if (tid == kScanThreads - 1u) { totals[0] = start_a + sa[tid]; totals[1] = start_b + sb[tid]; }
}
}  // namespace
