// bv_text_job.hip -- batchfile rows parsed a few files at a time: the parse job (bv_engine_text_job_begin / _add / _finish,
// include/basevar_amd_text_job.h; the contract is INTEGRATION.md section 2q).
//
// bv_text_parse_kernel (bv_text.hip) needs one thing of all files at once: file 0's row of the position, to which CHROM, POS and
// REF of every row are held.  Everything else it leaves is additive over files -- depth an atomicAdd, pstate an atomicOr, pmax an
// atomicMax per position, the cells of file f in its own columns.  Here an add brings the rows of K adjacent files for all P
// positions of the job.  In place of file 0's row stands the position's head, the first 512 bytes at most of the first row added
// for it, through its third tab: bv_text_job_head_kernel captures it in front of the parse kernel of the position's first add
// (adds are serial on the stream, so no two adds race for it), and bv_text_job_parse_kernel walks every row as
// bv_text_parse_kernel does (bv_text_row_walk_body.h) against it.  After the last add the strand kernel, the positions'
// states and the token list's pack run as they do behind bv_engine_text_parse.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/basevar_amd_text_job.h"
#include "bv_text_rows.h"
#include "bv_text_tokens_walk.h"

using namespace bv_impl;

namespace {

struct TextJobArgs {
    TextParseArgs a;           // row_beg, row_end, row_first and n_rows_chunk count the add's rows; everything else is the job's
    const char *heads;         // [P][kMaxPrefix]
    const uint32_t *head_len;  // [P]
    uint32_t first_file, K;    // the add holds files [first_file, first_file + K)
};

// One wave per row of the add's chunk; four rows per workgroup.  Row l = p * K + k of the add is row p * n_files + first_file + k
// of the job.
__global__ __launch_bounds__(256) void bv_text_job_parse_kernel(TextJobArgs j) {
    const TextParseArgs &a = j.a;
    const uint32_t first_file = j.first_file, K = j.K;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t local = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (local >= a.n_rows_chunk) return;
    const uint32_t l = a.row_first + local;
    const uint32_t p = l / K, f = first_file + (l - p * K), r = p * a.n_files + f;
    const char *row = a.text + (a.row_beg[l] - a.chunk_base);
    const char *row0 = j.heads + (size_t)p * kMaxPrefix;  // the position's head
    const uint32_t len = (uint32_t)(a.row_end[l] - a.row_beg[l]);  // the last byte is '\n' (checked by the host)
    const uint32_t len0 = j.head_len[p];

#include "bv_text_row_walk_body.h"
}

// In front of it: one wave per position of the chunk; a position without a head (length 0: a row has a byte at least) takes the
// head of row (p, 0) of the add -- its bytes through the third tab, or its first kMaxPrefix if the tab is not among them.
struct TextJobHeadArgs {
    const char *text;
    const uint64_t *row_beg, *row_end;  // of the add's rows
    uint64_t chunk_base;
    uint32_t pos_first, n_pos, K;
    char *heads;
    uint32_t *head_len;
};
__global__ __launch_bounds__(256) void bv_text_job_head_kernel(TextJobHeadArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t local = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (local >= a.n_pos) return;
    const uint32_t p = a.pos_first + local;
    if (a.head_len[p] != 0) return;  // captured by an earlier add
    const size_t l = (size_t)p * a.K;
    const char *row = a.text + (a.row_beg[l] - a.chunk_base);
    const uint32_t lim = (uint32_t)min(a.row_end[l] - a.row_beg[l], (uint64_t)kMaxPrefix);
    char *head = a.heads + (size_t)p * kMaxPrefix;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t tabs = 0, cut = lim;
    for (uint32_t b = 0; b < lim; b += 64u) {
        const uint32_t i = b + lane;
        const bool valid = i < lim;
        const char c = valid ? row[i] : '\0';
        const bool tab = valid && c == '\t';
        const uint64_t T = __ballot(tab);
        const uint64_t third = __ballot(tab && tabs + (uint32_t)__popcll(T & lt) == 2u);  // the lane of the row's third tab
        const uint32_t stop = third ? (uint32_t)__ffsll((unsigned long long)third) - 1u : 63u;
        if (valid && lane <= stop) head[i] = c;
        if (third) { cut = b + stop + 1u; break; }
        tabs += (uint32_t)__popcll(T);
    }
    if (lane == 0) a.head_len[p] = cut;
}

// ---- the add's indel tokens (the mode of basevar_amd_text_tokens.h): count, scan and write of bv_text_tokens.hip in their
// strided form.  The add's rows are K out of every n_files rows of the batch: the counts and the places are kept at the rows'
// indices in the batch, where the final scan and bv_tt_pack_kernel find them in (position, file) order whatever the adds' order;
// the scan of a chunk runs over the add's rows in the add's order.
struct TokJobArgs {
    TokArgs a;  // row_beg, row_end and row_first, n_rows count the add's rows; everything else is the batch's
    uint32_t first_file, K;
};
__global__ __launch_bounds__(256) void bv_tt_count_job_kernel(TokJobArgs j) {
    const uint32_t local = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (local >= j.a.n_rows) return;
    const uint32_t l = j.a.row_first + local;
    walk_row<false>(j.a, job_row(l, j.a.n_files, j.first_file, j.K), l, threadIdx.x & 63u);
}
__global__ __launch_bounds__(256) void bv_tt_write_job_kernel(TokJobArgs j) {
    const uint32_t local = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (local >= j.a.n_rows) return;
    const uint32_t l = j.a.row_first + local;
    walk_row<true>(j.a, job_row(l, j.a.n_files, j.first_file, j.K), l, threadIdx.x & 63u);
}
__global__ __launch_bounds__(kScanThreads) void bv_tt_scan_job_kernel(const uint32_t *ca, const uint32_t *cb, uint32_t F, uint32_t first, uint32_t n,
                                                                      uint64_t start_a, uint64_t start_b, uint64_t *out_a, uint64_t *out_b, uint64_t *totals,
                                                                      uint32_t first_file, uint32_t K) {
    scan_rows<true>(ca, cb, nullptr, F, first, n, start_a, start_b, out_a, out_b, totals, first_file, K);
}
TokJobArgs tok_job_args(const BvTextTokRows &rows, const BvTextTokStore &s) {
    TokJobArgs j;
    j.a.text = rows.text; j.a.row_beg = rows.row_beg; j.a.row_end = rows.row_end; j.a.rowflag = rows.rowflag; j.a.foff = rows.foff;
    j.a.chunk_base = rows.chunk_base; j.a.row_first = rows.row_first; j.a.n_rows = rows.n_rows; j.a.n_files = rows.n_files;
    j.a.cnt_tok = s.cnt_tok; j.a.cnt_txt = s.cnt_txt; j.a.base_tok = s.base_tok; j.a.base_txt = s.base_txt;
    j.a.tok = reinterpret_cast<bv_tt_token *>(s.tok); j.a.ttext = s.ttext;
    j.first_file = rows.first_file; j.K = rows.add_files;
    return j;
}

uint32_t *head_len_of(BvTextState *t, uint32_t P) { return reinterpret_cast<uint32_t *>(t->d_heads + up256((size_t)P * kMaxPrefix)); }

int job_add(bv_engine *e, BvTextState *t, const bv_text_rows *rows, uint32_t first_file, uint8_t *row_flag, hipStream_t st) {
    BvTextJob &J = t->job;
    const ParseBufs &pb = J.pb;
    const uint32_t P = J.P, F = J.F, K = rows->n_files;
    const size_t RK = (size_t)P * K;
    BV_HIP(e, hipSetDevice(t->device));
    BV_HIP(e, hipMemcpyAsync(pb.d_off, rows->row_off, 8 * (RK + 1), hipMemcpyHostToDevice, st));
    // the chunks: whole positions, at most kChunkBytes (or one position, if it is longer)
    size_t need = 0;
    for (uint32_t p = 0; p < P; ++p) need = std::max<size_t>(need, rows->row_off[(size_t)(p + 1) * K] - rows->row_off[(size_t)p * K]);
    const size_t total = rows->row_off[RK] - rows->row_off[0];
    const size_t chunk_bytes = chunk_limit_from_env("BASEVAR_AMD_TEXT_CHUNK_BYTES", kChunkBytes);
    ChunkStage &cst = t->chunks;
    int rc = chunk_stage_begin(e, cst, st);  // (with it, the pageable upload above is complete)
    if (rc == BV_OK) rc = chunk_stage_reserve(e, cst, std::max(up256(need), std::min(chunk_bytes, up256(total))));
    if (rc != BV_OK) return rc;
    unsigned k = 0;
    for (uint32_t p0 = 0; p0 < P; ++k) {
        const uint64_t base = rows->row_off[(size_t)p0 * K];
        uint32_t p1 = p0 + 1;
        while (p1 < P && rows->row_off[(size_t)(p1 + 1) * K] - base <= cst.cap) ++p1;
        const size_t bytes = rows->row_off[(size_t)p1 * K] - base;
        const unsigned s = k & 1u;
        if ((rc = chunk_stage_fill(e, cst, s)) != BV_OK) return rc;
        std::memcpy(cst.slot[s].h, rows->text + base, bytes);
        if ((rc = chunk_stage_upload(e, cst, s, bytes, st)) != BV_OK) return rc;
        TextJobArgs j;
        TextParseArgs &a = j.a;
        a.text = reinterpret_cast<const char *>(cst.slot[s].d); a.row_beg = pb.d_off; a.row_end = pb.d_off + 1; a.foff = pb.foff; a.fsamp = pb.fsamp;
        a.chunk_base = base; a.row_first = p0 * K; a.n_rows_chunk = (p1 - p0) * K; a.n_files = F; a.pitch = pb.pitch;
        a.bs = pb.bs; a.q = pb.q; a.mq = pb.mq; a.st = pb.stp; a.ref = pb.ref; a.rowflag = pb.rowflag; a.rp = pb.rp;
        a.depth = pb.depth; a.pstate = pb.pstate; a.pmax = pb.pmax;
        j.heads = reinterpret_cast<const char *>(t->d_heads); j.head_len = head_len_of(t, P); j.first_file = first_file; j.K = K;
        const TextJobHeadArgs h{a.text, a.row_beg, a.row_end, base, p0, p1 - p0, K, reinterpret_cast<char *>(t->d_heads), head_len_of(t, P)};
        hipLaunchKernelGGL(bv_text_job_head_kernel, dim3((h.n_pos + 3u) / 4u), dim3(256), 0, st, h);
        hipLaunchKernelGGL(bv_text_job_parse_kernel, dim3((a.n_rows_chunk + 3u) / 4u), dim3(256), 0, st, j);
        BV_HIP(e, hipGetLastError());
        // (the mode of basevar_amd_text_tokens.h: the chunk's indel tokens, while its text is here)
        if ((rc = bv_text_tokens_rows(e, BvTextTokRows{a.text, a.row_beg, a.row_end, pb.rowflag, pb.foff, base, a.row_first, a.n_rows_chunk, F, first_file, K},
                                      st)) != BV_OK)
            return rc;
        if ((rc = chunk_stage_done(e, cst, s, st)) != BV_OK) return rc;
        p0 = p1;
    }
    // the add's rows of rowflag: K out of every F
    if (row_flag) BV_HIP(e, hipMemcpy2DAsync(row_flag, K, pb.rowflag + first_file, F, K, P, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));  // the text has been consumed
    return BV_OK;
}

}  // namespace

namespace bv_impl {
void text_job_tokens_count_scan(const BvTextTokRows &rows, const BvTextTokStore &s, uint64_t run_tok, uint64_t run_txt, hipStream_t st) {
    hipLaunchKernelGGL(bv_tt_count_job_kernel, dim3((rows.n_rows + 3u) / 4u), dim3(256), 0, st, tok_job_args(rows, s));
    hipLaunchKernelGGL(bv_tt_scan_job_kernel, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t *)s.cnt_tok, (const uint32_t *)s.cnt_txt, rows.n_files,
                       rows.row_first, rows.n_rows, run_tok, run_txt, s.base_tok, s.base_txt, s.totals, rows.first_file, rows.add_files);
}
void text_job_tokens_write(const BvTextTokRows &rows, const BvTextTokStore &s, hipStream_t st) {
    hipLaunchKernelGGL(bv_tt_write_job_kernel, dim3((rows.n_rows + 3u) / 4u), dim3(256), 0, st, tok_job_args(rows, s));
}
}  // namespace bv_impl

extern "C" {

int bv_engine_text_job_begin(bv_engine *e, uint32_t n_positions, uint32_t n_files, const uint32_t *file_samples, const uint8_t *group_id,
                             uint32_t n_groups, void *stream_) {
    const char *who = "bv_engine_text_job_begin";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, std::string(who) + ": null engine");
    if (!file_samples) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null file_samples");
    if (n_positions == 0 || n_files == 0) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": n_positions and n_files must be > 0");
    if (n_positions > e->cfg.max_sites) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": n_positions exceeds cfg.max_sites");
    uint64_t n_samples = 0;
    int rc = text_check_samples_groups(e, who, file_samples, n_files, group_id, n_groups, &n_samples);
    if (rc != BV_OK) return rc;
    BvTextState *t = text_state(e);
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    BvTextJob &J = t->job;
    rc = text_parse_begin(e, t, n_positions, n_files, file_samples, (uint32_t)n_samples, st, &J.pb);  // (an open job is abandoned)
    if (rc != BV_OK) return rc;
    const size_t o_len = up256((size_t)n_positions * kMaxPrefix);
    rc = grow_device(e, &t->d_heads, &t->heads_bytes, o_len + up256(4ull * n_positions));
    if (rc != BV_OK) return rc;
    BV_HIP(e, hipMemsetAsync(t->d_heads + o_len, 0, 4ull * n_positions, st));
    BV_HIP(e, hipStreamSynchronize(st));  // (file_samples has been read)
    J.P = n_positions; J.F = n_files; J.n_samples = (uint32_t)n_samples; J.n_groups = n_groups; J.n_added = 0;
    J.file_samples.assign(file_samples, file_samples + n_files);
    J.added.assign(n_files, 0);
    J.has_gid = group_id != nullptr;
    if (group_id) J.group_id.assign(group_id, group_id + n_samples);
    else J.group_id.clear();
    J.tokens = bv_text_tokens_on(e);
    J.open = true;
    return BV_OK;
}

int bv_engine_text_job_add(bv_engine *e, const bv_text_rows *rows, uint32_t first_file, uint8_t *row_flag, void *stream_) {
    const char *who = "bv_engine_text_job_add";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, std::string(who) + ": null engine");
    BvTextState *t = e->text;
    if (!t || !t->job.open) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": no open job (bv_engine_text_job_begin)");
    if (!rows) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null rows");
    int rc = text_check_rows_head(e, who, rows);
    if (rc != BV_OK) return rc;
    BvTextJob &J = t->job;
    if (rows->n_positions != J.P)
        return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": n_positions is " + std::to_string(rows->n_positions) + ", the job's is " + std::to_string(J.P));
    if ((uint64_t)first_file + rows->n_files > J.F)
        return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": files " + std::to_string(first_file) + " .. " + std::to_string((uint64_t)first_file + rows->n_files) +
                                               " reach beyond the job's " + std::to_string(J.F) + " files");
    for (uint32_t k = 0; k < rows->n_files; ++k) {
        if (J.added[first_file + k]) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": file " + std::to_string(first_file + k) + " was added before");
        if (rows->file_samples[k] != J.file_samples[first_file + k])
            return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": file_samples of file " + std::to_string(first_file + k) + " is " +
                                                   std::to_string(rows->file_samples[k]) + ", the job's is " + std::to_string(J.file_samples[first_file + k]));
    }
    if ((rc = text_check_rows_off(e, who, rows)) != BV_OK) return rc;
    if (J.tokens != bv_text_tokens_on(e)) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": the token mode changed since the job's begin");
    rc = job_add(e, t, rows, first_file, row_flag, stream_ ? (hipStream_t)stream_ : e->stream);
    if (rc != BV_OK) {
        J.open = false;
        return rc;
    }
    for (uint32_t k = 0; k < rows->n_files; ++k) J.added[first_file + k] = 1;
    J.n_added += rows->n_files;
    return BV_OK;
}

int bv_engine_text_job_finish(bv_engine *e, uint8_t *row_state, void *stream_) {
    const char *who = "bv_engine_text_job_finish";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, std::string(who) + ": null engine");
    BvTextState *t = e->text;
    if (!t || !t->job.open) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": no open job (bv_engine_text_job_begin)");
    if (!row_state) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null row_state");
    BvTextJob &J = t->job;
    if (J.n_added != J.F) {
        uint32_t f = 0;
        while (J.added[f]) ++f;
        return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": " + std::to_string(J.F - J.n_added) + " of the job's " + std::to_string(J.F) +
                                               " files are missing, file " + std::to_string(f) + " the first");
    }
    if (J.tokens != bv_text_tokens_on(e)) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": the token mode changed since the job's begin");
    J.open = false;
    BV_HIP(e, hipSetDevice(t->device));
    const int rc = text_parse_finish(e, t, J.P, J.F, J.n_samples, J.has_gid ? J.group_id.data() : nullptr, J.n_groups, row_state,
                                     stream_ ? (hipStream_t)stream_ : e->stream, J.pb);
    if (rc != BV_OK) t->parsed = false;
    return rc;
}

}  // extern "C"
