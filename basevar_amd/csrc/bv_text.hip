// bv_text.hip -- batchfile text rows parsed on the device (bv_engine_text_parse / bv_engine_text_submit, include/basevar_amd.h;
// the contract is INTEGRATION.md section 2e).
//
// The reference reads one row from every batchfile per position and splits its columns token by token on the host
// (src/basetype_caller.cpp:586-611, 686-740).  Here the rows of a whole batch go to the device as they are: one wave per
// (position, file) row walks the row 64 bytes at a time, finds the column and token of every byte with 64-bit ballots of its
// tabs and spaces, and the lane that holds a token's first byte decodes it into the slab planes the calling kernels read.
// File f's tokens land at sample offset file_samples[0] + ... + file_samples[f - 1] of the position's row.
//
// The device takes a row only in the narrow form every well-formed batchfile has (9 fields; CHROM, POS and REF byte-equal to
// file 0's row; decimal Depth and POS of at most 9 digits; exactly file_samples[f] tokens per sample column; mapq 1-3 digits
// <= 255; base one of A C G T N or a '+'/'-' token; quality one character; rank 1-5 digits <= 65,535; strand '+', '-' or '.'; a
// covered base never with '.').  For such a row the host reader (batchfile_fast.hpp, parse_site_rows_fast) writes the same
// bytes; anything else makes the whole position "host" and the caller re-reads it with that reader, which keeps every odd
// case and error message of the reference.  Positions whose Depth fields sum to 0 are skipped (caller.cpp:718) -- before any
// token is looked at, as the host reader does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/basevar_amd_bgzf.h"
#include "../../include/basevar_amd_text_tokens.h"
#include "../../include/basevar_amd_region.h"
#include "../../include/basevar_amd_diag.h"
#include "bv_inflate_core.h"
#include "bv_text_rows.h"
#include "bv_text_region_core.h"

using namespace bv_impl;

namespace {

// One wave per (position, file) row; four rows per workgroup.
__global__ __launch_bounds__(256) void bv_text_parse_kernel(TextParseArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t local = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (local >= a.n_rows_chunk) return;
    const uint32_t r = a.row_first + local;
    const uint32_t p = r / a.n_files, f = r - p * a.n_files;
    const uint32_t r0 = p * a.n_files;  // file 0's row of the same position
    const char *row = a.text + (a.row_beg[r] - a.chunk_base);
    const char *row0 = a.text + (a.row_beg[r0] - a.chunk_base);
    const uint32_t len = (uint32_t)(a.row_end[r] - a.row_beg[r]);  // the last byte is '\n' (checked by the host / the line index)
    const uint32_t len0 = (uint32_t)(a.row_end[r0] - a.row_beg[r0]);

#include "bv_text_row_walk_body.h"
}

// After the last chunk: the strand of every covered call goes into its cell (REV for '-'); a covered call with strand '.'
// makes the position "host" (the reference refuses it: basetype.cpp:272).  One workgroup per position.
__global__ __launch_bounds__(256) void bv_text_strand_kernel(uint8_t *bs, const uint8_t *st, const uint32_t *depth, uint32_t *pstate,
                                                             uint64_t pitch, uint32_t n_samples) {
    const uint32_t p = blockIdx.x;
    if (pstate[p] != 0 || depth[p] == 0) return;
    uint8_t *row = bs + (size_t)p * pitch;
    const uint8_t *srow = st + (size_t)p * pitch;
    uint32_t bad = 0;
    for (uint32_t c = threadIdx.x; c < n_samples; c += blockDim.x) {
        const uint8_t b = row[c];
        if (b & BV_CELL_NOCALL) continue;
        const uint8_t s = srow[c];
        if (s == 2u) bad = 1;
        else if (s == 1u) row[c] = (uint8_t)(b | BV_CELL_REV);
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) pstate[p] |= kTokenFail;
}

// Submit: output row j takes parsed row src[j] >= 0, or host row -src[j] - 1 of the caller's slab (staged to hq..); ranks are
// written tagged when `tagged` (BV_RPR_TAGGED, what SlabBuilder::tag_ranks gives).  One workgroup per output row.
struct TextGatherArgs {
    const int32_t *src;
    const uint8_t *pbs, *pq, *pmq, *pref;
    const uint16_t *prp;
    uint64_t ppitch;
    const uint8_t *hbs, *hq, *hmq, *href;
    const uint16_t *hrp;
    uint64_t hpitch;
    uint8_t *bs, *q, *mq, *ref;
    uint16_t *rp;
    uint64_t pitch;
    uint32_t n_samples, tagged;
};
__global__ __launch_bounds__(256) void bv_text_gather_kernel(TextGatherArgs a) {
    const uint32_t j = blockIdx.x;
    const int32_t s = a.src[j];
    const bool dev = s >= 0;
    const size_t so = dev ? (size_t)s * a.ppitch : (size_t)(-s - 1) * a.hpitch;
    const uint8_t *sbs = (dev ? a.pbs : a.hbs) + so, *sq = (dev ? a.pq : a.hq) + so, *smq = (dev ? a.pmq : a.hmq) + so;
    const uint16_t *srp = (dev ? a.prp : a.hrp) + so;
    const size_t d = (size_t)j * a.pitch;
    for (uint32_t c = threadIdx.x; c < (uint32_t)a.pitch; c += blockDim.x) {
        const bool in = c < a.n_samples;
        const uint8_t b = in ? sbs[c] : (uint8_t)BV_CELL_N;
        const uint16_t r = in ? srp[c] : (uint16_t)0;
        a.bs[d + c] = b;
        a.q[d + c] = in ? sq[c] : (uint8_t)0;
        a.mq[d + c] = in ? smq[c] : (uint8_t)0;
        a.rp[d + c] = a.tagged ? BV_RPR_TAGGED((uint32_t)b, (uint32_t)r) : r;
    }
    if (threadIdx.x == 0) a.ref[j] = dev ? a.pref[s] : a.href[-s - 1];
}

// ---- rows that arrive compressed (bv_engine_text_parse_bgzf, include/basevar_amd_bgzf.h): the line index over the inflated runs.
// File f's run lies at text[base .. base + len), with one spare byte behind it that holds '\n': where the runs reach the ends of
// their files and the last line has no line break, the spare byte is its line break.  One wave per 16 KiB tile of a run counts
// the line ends (bv_text_line_count_kernel), one thread per file sums its tiles and takes the minimum of the files' complete
// lines (bv_text_line_scan_kernel), and the tiles are walked again to write every taken row's begin and end
// (bv_text_line_scatter_kernel).
constexpr uint32_t kLineTile = 16384;
struct LineFile {
    uint64_t base, len, skip;  // the run inside the text; inflated bytes before the file's first row
    uint32_t skip_lines;       // further lines before it
    uint32_t tile_first, n_tiles, reserved_;
};

__device__ __forceinline__ uint32_t line_file_of(const LineFile *fl, uint32_t F, uint32_t tile) {
    uint32_t lo = 0, hi = F - 1u;  // the last file whose first tile is <= tile (files without a tile share the next one's)
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) / 2u;
        if (fl[mid].tile_first <= tile) lo = mid; else hi = mid - 1u;
    }
    return lo;
}
// bytes of the run that the index looks at: the run, and the spare '\n' where it ends an unterminated last line
__device__ __forceinline__ uint64_t line_run_end(const char *text, const LineFile &L, uint32_t at_end) {
    return L.len + ((at_end && L.len > L.skip && text[L.base + L.len - 1] != '\n') ? 1u : 0u);
}

__global__ __launch_bounds__(64) void bv_text_line_pad_kernel(char *text, const LineFile *fl, uint32_t F) {
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f < F) text[fl[f].base + fl[f].len] = '\n';
}

__global__ __launch_bounds__(64) void bv_text_line_count_kernel(const char *text, const LineFile *fl, uint32_t F, uint32_t at_end, uint32_t *tile_cnt) {
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    const LineFile L = fl[line_file_of(fl, F, tile)];
    const uint64_t end = line_run_end(text, L, at_end);
    const uint64_t lo = L.skip + (uint64_t)(tile - L.tile_first) * kLineTile, hi = lo + kLineTile < end ? lo + kLineTile : end;
    uint32_t cnt = 0;
    for (uint64_t x = lo + lane; x < hi; x += 64u) cnt += text[L.base + x] == '\n';
    for (int o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, o);
    if (lane == 0) tile_cnt[tile] = cnt;
}

// tile_cnt -> exclusive prefix inside each file; *n_pos (set to the caller's limit before) -> min over the files' lines
__global__ __launch_bounds__(256) void bv_text_line_scan_kernel(const LineFile *fl, uint32_t F, uint32_t *tile_cnt, uint32_t *n_pos) {
    for (uint32_t f = threadIdx.x; f < F; f += 256u) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < fl[f].n_tiles; ++k) {
            const uint32_t c = tile_cnt[fl[f].tile_first + k];
            tile_cnt[fl[f].tile_first + k] = run;
            run += c;
        }
        atomicMin(n_pos, run > fl[f].skip_lines ? run - fl[f].skip_lines : 0u);
    }
}

__global__ __launch_bounds__(64) void bv_text_line_scatter_kernel(const char *text, const LineFile *fl, uint32_t F, uint32_t at_end,
                                                                  const uint32_t *tile_pre, uint32_t P, uint64_t *row_beg, uint64_t *row_end) {
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    const uint32_t f = line_file_of(fl, F, tile);
    const LineFile L = fl[f];
    const uint64_t end = line_run_end(text, L, at_end);
    const uint64_t lo = L.skip + (uint64_t)(tile - L.tile_first) * kLineTile, hi = lo + kLineTile < end ? lo + kLineTile : end;
    if (tile == L.tile_first && L.skip_lines == 0 && lane == 0) row_beg[f] = L.base + L.skip;
    uint32_t ord = tile_pre[tile];  // line ends of this run before the tile
    const uint64_t lt = (1ull << lane) - 1ull;
    for (uint64_t x0 = lo; x0 < hi; x0 += 64u) {
        const uint64_t x = x0 + lane;
        const bool nl = x < hi && text[L.base + x] == '\n';
        const uint64_t B = __ballot(nl);
        if (nl) {
            // line end number j of the run ends row j - skip_lines and begins the next one
            const int64_t q = (int64_t)(ord + (uint32_t)__popcll(B & lt)) - (int64_t)L.skip_lines;
            if (q >= 0 && q < (int64_t)P) row_end[(size_t)q * F + f] = L.base + x + 1u;
            if (q + 1 >= 0 && q + 1 < (int64_t)P) row_beg[(size_t)(q + 1) * F + f] = L.base + x + 1u;
        }
        ord += (uint32_t)__popcll(B);
    }
}

// ---- the rows of a region (bv_engine_text_parse_bgzf_region, include/basevar_amd_region.h; the definition and the walk stand at
// the head of bv_text_region_core.h).  Between the line scan and the scatter: one wave per tile reads the head of every line
// that begins behind one of the tile's line breaks -- the lane that holds the line break reads on inside the run, across the
// tile's edge where the head crosses it -- and folds the steps' masks into the tile's summary (bv_text_region_head_kernel); one
// thread per file folds its tiles, and one thread decides P, region_done and the refusal (bv_text_region_combine_kernel).  The
// scatter then runs on a copy of the LineFiles with skip_lines + first[f], for P + 1 rows: the begin of row (P, f) is the
// cursor.  bv_text_region_pos_kernel holds POS of every taken row to file 0's.
__global__ __launch_bounds__(64) void bv_text_region_head_kernel(const char *text, const LineFile *fl, uint32_t F, uint32_t at_end, const uint32_t *tile_pre,
                                                                 bv_tr_region rg, bv_tr_tile *out) {
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    const LineFile L = fl[line_file_of(fl, F, tile)];
    const uint64_t end = line_run_end(text, L, at_end);
    const uint64_t lo = L.skip + (uint64_t)(tile - L.tile_first) * kLineTile, hi = lo + kLineTile < end ? lo + kLineTile : end;
    const char *run = text + L.base;
    bv_tr_tile t = bv_tr_tile_init();
    const uint32_t pre = tile_pre[tile];  // line breaks of this run before the tile
    uint32_t ord = pre, pos = 0;
    if (tile == L.tile_first && L.skip_lines == 0) {  // the run's first line: a step of its own
        const uint32_t c = lane == 0 ? bv_tr_head(run + L.skip, end - L.skip, rg, &pos) : 0u;
        bv_tr_step(t, 1ull, __ballot((c & BV_TR_REACHED) != 0), __ballot(lane == 0 && !(c & BV_TR_IN)), __ballot((c & BV_TR_MAL) != 0), 0u);
    }
    const uint64_t lt = (1ull << lane) - 1ull;
    for (uint64_t x0 = lo; x0 < hi; x0 += 64u) {
        const uint64_t x = x0 + lane;
        const bool nl = x < hi && run[x] == '\n';
        const uint64_t B = __ballot(nl);
        // line break number j of the run begins line j + 1, whose ordinal is j + 1 - skip_lines
        const bool has = nl && ord + (uint32_t)__popcll(B & lt) + 1u >= L.skip_lines;
        const uint64_t LS = __ballot(has);
        if (LS) {
            const uint32_t c = has ? bv_tr_head(run + x + 1u, end - (x + 1u), rg, &pos) : 0u;
            const uint32_t q0 = ord + (uint32_t)__popcll(B & bv_tr_below(bv_tr_low(LS))) + 1u - L.skip_lines;
            bv_tr_step(t, LS, __ballot(has && (c & BV_TR_REACHED)), __ballot(has && !(c & BV_TR_IN)), __ballot(has && (c & BV_TR_MAL)), q0);
        }
        ord += (uint32_t)__popcll(B);
    }
    t.cnt = ord - pre;
    if (lane == 0) out[tile] = t;
}

// files[f], the LineFile the scatter takes for file f, and *res
__global__ __launch_bounds__(256) void bv_text_region_combine_kernel(const LineFile *fl, uint32_t F, const bv_tr_tile *tiles, uint32_t cap, uint32_t at_end,
                                                                    bv_tr_file *files, LineFile *fl_sel, bv_tr_result *res) {
    for (uint32_t f = threadIdx.x; f < F; f += 256u) {
        LineFile L = fl[f];
        bv_tr_file s = bv_tr_file_init();
        uint32_t breaks = 0;
        for (uint32_t k = 0; k < L.n_tiles; ++k) {
            const bv_tr_tile t = tiles[L.tile_first + k];
            bv_tr_file_add(s, t);
            breaks += t.cnt;
        }
        bv_tr_file_finish(s, breaks, L.skip_lines);
        files[f] = s;
        L.skip_lines += s.first;
        fl_sel[f] = L;
    }
    __syncthreads();
    if (threadIdx.x == 0) *res = bv_tr_decide(files, F, cap, at_end);
}

// *err (set to BV_TR_NONE before) -> the lowest row r = p * F + f whose POS is not row (p, 0)'s
__global__ __launch_bounds__(256) void bv_text_region_pos_kernel(const char *text, const uint64_t *row_beg, const uint64_t *row_end, uint32_t R, uint32_t F,
                                                                uint32_t *err) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= R) return;
    const uint32_t r0 = r - r % F;
    if (r == r0) return;
    const bv_tr_region any{nullptr, 0u, 0u, 0u};  // (heads of taken rows are well-formed: only POS is read)
    uint32_t pos = 0, pos0 = 0;
    (void)bv_tr_head(text + row_beg[r], row_end[r] - row_beg[r], any, &pos);
    (void)bv_tr_head(text + row_beg[r0], row_end[r0] - row_beg[r0], any, &pos0);
    if (pos != pos0) atomicMin(err, r);
}

// ---- bv_engine_text_rows_fetch: how much of every row the host still needs, then the bytes
__global__ __launch_bounds__(256) void bv_text_fetch_len_kernel(const char *text, const uint64_t *row_beg, const uint64_t *row_end, const uint8_t *pos_state,
                                                                const uint8_t *rowflag, uint32_t R, uint32_t F, uint32_t heads, uint32_t *len) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= R) return;
    const uint32_t p = r / F, f = r - p * F;
    const uint8_t s = pos_state[p];
    const uint32_t n = (uint32_t)(row_end[r] - row_beg[r]) - 1u;  // without the line break
    uint32_t out = 0;
    if (s & BV_TEXT_SKIP) {
        out = 0;
    } else if ((s & BV_TEXT_HOST) || (!heads && (rowflag[r] & BV_TEXT_INDEL))) {  // (heads: bv_engine_text_heads_fetch)
        out = n;
    } else if (f == 0) {  // CHROM \t POS \t REF \t Depth \t
        const char *row = text + row_beg[r];
        uint32_t tabs = 0, i = 0;
        for (; i < n && tabs < 4u; ++i) tabs += row[i] == '\t';
        out = i;
    }
    len[r] = out;
}
__global__ __launch_bounds__(256) void bv_text_fetch_copy_kernel(const char *text, const uint64_t *row_beg, const uint32_t *len, const uint64_t *off,
                                                                 uint32_t R, uint8_t *out) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (r >= R) return;
    const char *row = text + row_beg[r];
    uint8_t *o = out + off[r];
    for (uint32_t i = lane; i < len[r]; i += 64u) o[i] = (uint8_t)row[i];
}

}  // namespace

bool bv_text_kept_rows(const BvTextState *t, BvKeptRows *rows) {
    if (!t || !t->sub_rows) return false;
    rows->cell = t->d_sub;
    rows->phred = t->d_sub + (size_t)t->sub_rows * t->sub_pitch;
    rows->pitch = t->sub_pitch; rows->n_rows = t->sub_rows; rows->n_samples = t->sub_samples;
    return true;
}

void bv_text_state_free(BvTextState *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    chunk_stage_free(t->chunks);
    for (uint8_t *b : {t->d_planes, t->d_sub, t->d_aux, t->d_misc, t->d_gid, t->d_btext, t->d_lines, t->d_fetch, t->d_rrows, t->d_heads})
        if (b) (void)hipFree(b);
    delete t;
}

namespace bv_impl {
// Sized, cleared (a parsed row is all 'N' where the text leaves nothing) and with the files' sample offsets in place.
int text_parse_begin(bv_engine *e, BvTextState *t, uint32_t P, uint32_t F, const uint32_t *file_samples, uint32_t n_samples, hipStream_t st,
                     ParseBufs *b) {
    const size_t R = (size_t)P * F;
    const uint64_t pitch = (n_samples + 255ull) & ~255ull;
    t->parsed = false;
    t->bgzf_rows = false;
    t->job.open = false;
    BV_HIP(e, hipSetDevice(t->device));
    // device buffers: planes, then the small per-position / per-row arrays
    const size_t cells = (size_t)P * pitch;
    int rc = grow_device(e, &t->d_planes, &t->planes_bytes, 6 * cells + up256(P));
    if (rc != BV_OK) return rc;
    const size_t o_pstate = up256(4ull * P), o_pmax = 2 * o_pstate, o_flag = 3 * o_pstate, o_off = o_flag + up256(R),
                 o_foff = o_off + up256(16 * (R + 1)), o_fs = o_foff + up256(4ull * F), aux = o_fs + up256(4ull * F);
    rc = grow_device(e, &t->d_aux, &t->aux_bytes, aux);
    if (rc != BV_OK) return rc;
    b->pitch = pitch;
    b->bs = t->d_planes; b->q = b->bs + cells; b->mq = b->q + cells; b->stp = b->mq + cells;
    b->rp = reinterpret_cast<uint16_t *>(b->stp + cells);
    b->ref = b->stp + 3 * cells;
    b->depth = reinterpret_cast<uint32_t *>(t->d_aux); b->pstate = reinterpret_cast<uint32_t *>(t->d_aux + o_pstate);
    b->pmax = reinterpret_cast<uint32_t *>(t->d_aux + o_pmax); b->foff = reinterpret_cast<uint32_t *>(t->d_aux + o_foff);
    b->fsamp = reinterpret_cast<uint32_t *>(t->d_aux + o_fs);
    b->rowflag = t->d_aux + o_flag;
    b->d_off = reinterpret_cast<uint64_t *>(t->d_aux + o_off);
    t->h_foff.resize(F);
    for (uint32_t f = 0, s = 0; f < F; s += file_samples[f], ++f) t->h_foff[f] = s;
    BV_HIP(e, hipMemsetAsync(b->bs, BV_CELL_N, cells, st));
    BV_HIP(e, hipMemsetAsync(b->q, 0, 3 * cells, st));  // q, mq, strand
    BV_HIP(e, hipMemsetAsync(b->rp, 0, 2 * cells, st));
    BV_HIP(e, hipMemsetAsync(t->d_aux, 0, o_off, st));
    BV_HIP(e, hipMemcpyAsync(b->foff, t->h_foff.data(), 4ull * F, hipMemcpyHostToDevice, st));
    BV_HIP(e, hipMemcpyAsync(b->fsamp, file_samples, 4ull * F, hipMemcpyHostToDevice, st));
    return bv_text_tokens_begin(e, P, F, st);
}

static int text_parse(bv_engine *e, BvTextState *t, const bv_text_rows *rows, const uint8_t *group_id, uint32_t n_groups, uint8_t *row_state,
                      hipStream_t st, uint32_t n_samples) {
    const uint32_t P = rows->n_positions, F = rows->n_files;
    const size_t R = (size_t)P * F;
    ParseBufs pb;
    int rc = text_parse_begin(e, t, P, F, rows->file_samples, n_samples, st, &pb);
    if (rc != BV_OK) return rc;
    const uint64_t pitch = pb.pitch;
    uint8_t *bs = pb.bs, *q = pb.q, *mq = pb.mq, *stp = pb.stp, *ref = pb.ref, *rowflag = pb.rowflag;
    uint16_t *rp = pb.rp;
    uint32_t *depth = pb.depth, *pstate = pb.pstate, *pmax = pb.pmax, *foff = pb.foff, *fsamp = pb.fsamp;
    uint64_t *d_off = pb.d_off;
    BV_HIP(e, hipMemcpyAsync(d_off, rows->row_off, 8 * (R + 1), hipMemcpyHostToDevice, st));
    // the chunks: whole positions, at most kChunkBytes (or one position, if it is longer)
    size_t need = 0;
    for (uint32_t p = 0; p < P; ++p) need = std::max<size_t>(need, rows->row_off[(size_t)(p + 1) * F] - rows->row_off[(size_t)p * F]);
    const size_t total = rows->row_off[R] - rows->row_off[0];
    const size_t chunk_bytes = chunk_limit_from_env("BASEVAR_AMD_TEXT_CHUNK_BYTES", kChunkBytes);
    ChunkStage &cst = t->chunks;
    rc = chunk_stage_begin(e, cst, st);  // (with it, the pageable uploads above are complete)
    if (rc == BV_OK) rc = chunk_stage_reserve(e, cst, std::max(up256(need), std::min(chunk_bytes, up256(total))));
    if (rc != BV_OK) return rc;
    unsigned k = 0;
    for (uint32_t p0 = 0; p0 < P; ++k) {
        const uint64_t base = rows->row_off[(size_t)p0 * F];
        uint32_t p1 = p0 + 1;
        while (p1 < P && rows->row_off[(size_t)(p1 + 1) * F] - base <= cst.cap) ++p1;
        const size_t bytes = rows->row_off[(size_t)p1 * F] - base;
        const unsigned s = k & 1u;
        if ((rc = chunk_stage_fill(e, cst, s)) != BV_OK) return rc;
        std::memcpy(cst.slot[s].h, rows->text + base, bytes);
        if ((rc = chunk_stage_upload(e, cst, s, bytes, st)) != BV_OK) return rc;
        TextParseArgs a;
        a.text = reinterpret_cast<const char *>(cst.slot[s].d); a.row_beg = d_off; a.row_end = d_off + 1; a.foff = foff; a.fsamp = fsamp; a.chunk_base = base;
        a.row_first = p0 * F; a.n_rows_chunk = (p1 - p0) * F; a.n_files = F; a.pitch = pitch;
        a.bs = bs; a.q = q; a.mq = mq; a.st = stp; a.ref = ref; a.rowflag = rowflag; a.rp = rp;
        a.depth = depth; a.pstate = pstate; a.pmax = pmax;
        hipLaunchKernelGGL(bv_text_parse_kernel, dim3((a.n_rows_chunk + 3u) / 4u), dim3(256), 0, st, a);
        BV_HIP(e, hipGetLastError());
        // (the mode of basevar_amd_text_tokens.h: the chunk's indel tokens, while its text is here)
        if ((rc = bv_text_tokens_rows(e, BvTextTokRows{a.text, a.row_beg, a.row_end, rowflag, foff, base, a.row_first, a.n_rows_chunk, F}, st)) != BV_OK) return rc;
        if ((rc = chunk_stage_done(e, cst, s, st)) != BV_OK) return rc;
        p0 = p1;
    }
    return text_parse_finish(e, t, P, F, n_samples, group_id, n_groups, row_state, st, pb);
}

// What every parse entry point asks of file_samples and group_id / n_groups; *n_samples = the samples of all files.
int text_check_samples_groups(bv_engine *e, const char *who, const uint32_t *file_samples, uint32_t F, const uint8_t *group_id, uint32_t n_groups,
                              uint64_t *n_samples) {
    *n_samples = 0;
    for (uint32_t f = 0; f < F; ++f) {
        if (file_samples[f] == 0) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": file_samples[f] == 0");
        *n_samples += file_samples[f];
    }
    if (*n_samples > e->cfg.max_samples)
        return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": the files hold more samples than cfg.max_samples");
    if (n_groups > BV_MAX_GROUPS || (n_groups > 0) != (group_id != nullptr))
        return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": group_id must be given with 0 < n_groups <= BV_MAX_GROUPS");
    return BV_OK;
}

// The strands into the cells, then what the host needs to know of every position.
int text_parse_finish(bv_engine *e, BvTextState *t, uint32_t P, uint32_t F, uint32_t n_samples, const uint8_t *group_id, uint32_t n_groups,
                      uint8_t *row_state, hipStream_t st, const ParseBufs &b) {
    const size_t R = (size_t)P * F;
    hipLaunchKernelGGL(bv_text_strand_kernel, dim3(P), dim3(256), 0, st, b.bs, (const uint8_t *)b.stp, (const uint32_t *)b.depth, b.pstate, b.pitch,
                       n_samples);
    BV_HIP(e, hipGetLastError());
    std::vector<uint32_t> h(3ull * P);
    BV_HIP(e, hipMemcpyAsync(h.data(), b.depth, 4ull * P, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipMemcpyAsync(h.data() + P, b.pstate, 4ull * P, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipMemcpyAsync(h.data() + 2ull * P, b.pmax, 4ull * P, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipMemcpyAsync(row_state, b.rowflag, R, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    // the position's state, in the host reader's order: field count / coordinates / Depth first, then Depth 0, then the tokens
    t->pos_state.assign(P, 0);
    t->pos_max_rank.assign(h.begin() + 2ull * P, h.end());
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t ps = h[P + p];
        const uint8_t s = (ps & kPrefixFail) ? BV_TEXT_HOST : h[p] == 0 ? BV_TEXT_SKIP : ps ? BV_TEXT_HOST : 0;
        t->pos_state[p] = s;
        for (uint32_t f = 0; f < F; ++f) {
            uint8_t &o = row_state[(size_t)p * F + f];
            o = s ? s : (uint8_t)(o & BV_TEXT_INDEL);
        }
    }
    t->n_pos = P; t->n_files = F; t->n_samples = n_samples; t->pitch = b.pitch; t->n_groups = n_groups;
    t->has_gid = group_id != nullptr;
    if (group_id) t->group_id.assign(group_id, group_id + n_samples);
    else t->group_id.clear();
    const int rc = bv_text_tokens_finish(e, t->pos_state.data(), P, F, st);
    if (rc != BV_OK) return rc;
    t->parsed = true;
    return BV_OK;
}

// What every call that takes a bv_text_rows asks of it: the pointers, reserved_ and the counts ...
int text_check_rows_head(bv_engine *e, const char *who, const bv_text_rows *rows) {
    if (!rows->text || !rows->row_off || !rows->file_samples)
        return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null text/row_off/file_samples");
    if (rows->reserved_) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": reserved_ must be zero");
    if (rows->n_positions == 0 || rows->n_files == 0)
        return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": n_positions and n_files must be > 0");
    return BV_OK;
}
// ... and the rows in order, inside the text, each ending in '\n'
int text_check_rows_off(bv_engine *e, const char *who, const bv_text_rows *rows) {
    const size_t R = (size_t)rows->n_positions * rows->n_files;
    for (size_t r = 0; r < R; ++r) {
        const uint64_t a = rows->row_off[r], b = rows->row_off[r + 1];
        if (b <= a || b > rows->text_bytes || rows->text[b - 1] != '\n')
            return fail(e, BV_ERR_INVALID_ARG,
                        std::string(who) + ": row " + std::to_string(r) + ": row_off outside text_bytes, out of order, or no final '\\n'");
        if (b - a > 0xFFFFFFFFull) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": a row is longer than 4 GiB");
    }
    return BV_OK;
}

BvTextState *text_state(bv_engine *e) { return engine_state(e, e->text); }
}  // namespace bv_impl

extern "C" {

int bv_engine_text_parse(bv_engine *e, const bv_text_rows *rows, const uint8_t *group_id, uint32_t n_groups, uint8_t *row_state,
                         void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_text_parse: null engine");
    if (!rows || !row_state) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_text_parse: null rows/row_state");
    int rc = text_check_rows_head(e, "bv_engine_text_parse", rows);
    if (rc != BV_OK) return rc;
    if (rows->n_positions > e->cfg.max_sites)
        return fail(e, BV_ERR_INVALID_ARG, "bv_engine_text_parse: n_positions exceeds cfg.max_sites");
    uint64_t n_samples = 0;
    rc = text_check_samples_groups(e, "bv_engine_text_parse", rows->file_samples, rows->n_files, group_id, n_groups, &n_samples);
    if (rc != BV_OK) return rc;
    if ((rc = text_check_rows_off(e, "bv_engine_text_parse", rows)) != BV_OK) return rc;
    BvTextState *t = engine_state(e, e->text);
    rc = text_parse(e, t, rows, group_id, n_groups, row_state, stream_ ? (hipStream_t)stream_ : e->stream, (uint32_t)n_samples);
    if (rc != BV_OK) t->parsed = false;
    return rc;
}

int bv_engine_text_submit(bv_engine *e, const uint8_t *row_state, const bv_slab *host_rows, uint32_t n_used, bv_site_result *out,
                          bv_group_result *gout, uint8_t *cell, uint8_t *phred, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_text_submit: null engine");
    BvTextState *t = e->text;
    if (!t || !t->parsed) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_text_submit: no bv_engine_text_parse before it");
    if (n_used > t->n_pos) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_text_submit: n_positions_used exceeds the parsed batch");
    // row_state (may be NULL: as the parse left it): the host reader may have skipped a "host" position (its Depth fields, read
    // its way, sum to 0); nothing else may change
    std::vector<uint8_t> state(t->pos_state.begin(), t->pos_state.begin() + n_used);
    if (row_state) {
        for (uint32_t p = 0; p < n_used; ++p) {
            const uint8_t s = (uint8_t)(row_state[(size_t)p * t->n_files] & (BV_TEXT_SKIP | BV_TEXT_HOST));
            if (s != state[p] && !(state[p] == BV_TEXT_HOST && s == BV_TEXT_SKIP))
                return fail(e, BV_ERR_INVALID_ARG, "bv_engine_text_submit: row_state of position " + std::to_string(p) +
                                                                 " differs from the parse (only HOST -> SKIP is allowed)");
            state[p] = s;
        }
    }
    uint32_t n_host = 0, n_out = 0;
    uint32_t max_rank = 0;
    for (uint32_t p = 0; p < n_used; ++p) {
        const uint8_t s = state[p];
        n_host += s == BV_TEXT_HOST;
        n_out += s != BV_TEXT_SKIP;
        if (s == 0) max_rank = std::max(max_rank, t->pos_max_rank[p]);
    }
    const uint32_t N = t->n_samples;
    if (n_host) {
        if (!host_rows || host_rows->n_sites != n_host || host_rows->n_samples != N || host_rows->pitch < N ||
            (host_rows->pitch & 15u) || host_rows->mem_kind != BV_MEM_HOST || host_rows->layout || host_rows->reserved_ || !host_rows->base_strand ||
            !host_rows->qual || !host_rows->mapq || !host_rows->rpr || !host_rows->ref_base)
            return fail(e, BV_ERR_INVALID_ARG,
                                  "bv_engine_text_submit: host_rows must hold the " + std::to_string(n_host) +
                                      " host positions as a plain BV_MEM_HOST slab of n_samples = " + std::to_string(N) +
                                      " with all five planes");
    } else if (host_rows && host_rows->n_sites) {
        return fail(e, BV_ERR_INVALID_ARG, "bv_engine_text_submit: host_rows given, but no position is marked host");
    }
    if (n_out && !out) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_text_submit: null out");
    if (n_out && t->n_groups && !gout) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_text_submit: n_groups > 0 needs gout");
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    t->parsed = false;  // one submit per parse, whatever happens below
    t->sub_rows = 0;
    if (n_out == 0) return BV_OK;
    BV_HIP(e, hipSetDevice(t->device));
    const uint64_t HP = n_host ? host_rows->pitch : 0;
    for (uint32_t h = 0; h < n_host; ++h) {  // the tagged layout needs every rank <= BV_RPR_TAG_MAX_RANK, host rows' too
        const uint16_t *r = host_rows->rpr + (size_t)h * HP;
        for (uint32_t c = 0; c < N; ++c) max_rank = std::max<uint32_t>(max_rank, r[c]);
    }
    const uint64_t P = t->pitch;
    const size_t cells = (size_t)n_out * P, hcells = (size_t)n_host * HP, G = t->n_groups;
    int rc = grow_device(e, &t->d_sub, &t->sub_bytes, 5 * cells + up256(n_out));
    if (rc != BV_OK) return rc;
    const size_t o_host = up256(4ull * n_out), o_out = o_host + up256(5 * hcells + n_host), o_gout = o_out + up256(sizeof(bv_site_result) * n_out),
                 misc = o_gout + up256(sizeof(bv_group_result) * n_out * G);
    rc = grow_device(e, &t->d_misc, &t->misc_bytes, misc);
    if (rc != BV_OK) return rc;
    std::vector<int32_t> src(n_out);
    for (uint32_t p = 0, j = 0, h = 0; p < n_used; ++p) {
        const uint8_t s = state[p];
        if (s == 0) src[j++] = (int32_t)p;
        else if (s == BV_TEXT_HOST) src[j++] = -(int32_t)(h++) - 1;
    }
    uint8_t *hb = t->d_misc + o_host;
    BV_HIP(e, hipMemcpyAsync(t->d_misc, src.data(), 4ull * n_out, hipMemcpyHostToDevice, st));
    if (n_host) {
        BV_HIP(e, hipMemcpyAsync(hb, host_rows->base_strand, hcells, hipMemcpyHostToDevice, st));
        BV_HIP(e, hipMemcpyAsync(hb + hcells, host_rows->qual, hcells, hipMemcpyHostToDevice, st));
        BV_HIP(e, hipMemcpyAsync(hb + 2 * hcells, host_rows->mapq, hcells, hipMemcpyHostToDevice, st));
        BV_HIP(e, hipMemcpyAsync(hb + 3 * hcells, host_rows->rpr, 2 * hcells, hipMemcpyHostToDevice, st));
        BV_HIP(e, hipMemcpyAsync(hb + 5 * hcells, host_rows->ref_base, n_host, hipMemcpyHostToDevice, st));
    }
    if (t->has_gid) {
        rc = grow_device(e, &t->d_gid, &t->gid_bytes, up256(N));
        if (rc != BV_OK) return rc;
        BV_HIP(e, hipMemcpyAsync(t->d_gid, t->group_id.data(), N, hipMemcpyHostToDevice, st));
    }
    const size_t pcells = (size_t)t->n_pos * P;
    const uint32_t tagged = max_rank <= BV_RPR_TAG_MAX_RANK ? 1u : 0u;
    TextGatherArgs a;
    a.src = reinterpret_cast<const int32_t *>(t->d_misc);
    a.pbs = t->d_planes; a.pq = a.pbs + pcells; a.pmq = a.pq + pcells;
    a.prp = reinterpret_cast<const uint16_t *>(t->d_planes + 4 * pcells); a.pref = t->d_planes + 6 * pcells; a.ppitch = P;
    a.hbs = hb; a.hq = hb + hcells; a.hmq = hb + 2 * hcells; a.hrp = reinterpret_cast<const uint16_t *>(hb + 3 * hcells);
    a.href = hb + 5 * hcells; a.hpitch = HP;
    a.bs = t->d_sub; a.q = a.bs + cells; a.mq = a.q + cells; a.rp = reinterpret_cast<uint16_t *>(a.mq + cells);
    a.ref = t->d_sub + 5 * cells; a.pitch = P; a.n_samples = N; a.tagged = tagged;
    hipLaunchKernelGGL(bv_text_gather_kernel, dim3(n_out), dim3(256), 0, st, a);
    BV_HIP(e, hipGetLastError());
    bv_slab s{};
    s.n_sites = n_out; s.n_samples = N; s.pitch = P;
    s.base_strand = a.bs; s.qual = a.q; s.mapq = a.mq; s.rpr = a.rp; s.ref_base = a.ref;
    s.group_id = G ? t->d_gid : nullptr; s.n_groups = (uint32_t)G;
    s.mem_kind = BV_MEM_DEVICE; s.layout = tagged ? BV_SLAB_RPR_TAGGED : 0u;
    bv_site_result *d_out = reinterpret_cast<bv_site_result *>(t->d_misc + o_out);
    bv_group_result *d_gout = G ? reinterpret_cast<bv_group_result *>(t->d_misc + o_gout) : nullptr;
    rc = bv_engine_submit(e, &s, d_out, d_gout, st);
    if (rc != BV_OK) return rc;
    rc = bv_engine_join(e, st);
    if (rc != BV_OK) return rc;
    BV_HIP(e, hipMemcpyAsync(out, d_out, sizeof(bv_site_result) * n_out, hipMemcpyDeviceToHost, st));
    if (G) BV_HIP(e, hipMemcpyAsync(gout, d_gout, sizeof(bv_group_result) * n_out * G, hipMemcpyDeviceToHost, st));
    if (cell) BV_HIP(e, hipMemcpy2DAsync(cell, N, a.bs, P, N, n_out, hipMemcpyDeviceToHost, st));
    if (phred) BV_HIP(e, hipMemcpy2DAsync(phred, N, a.q, P, N, n_out, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    t->sub_rows = n_out; t->sub_samples = N; t->sub_pitch = P; t->sub_layout = s.layout;  // (d_sub stands until the next submit, whatever is parsed meanwhile)
    return BV_OK;
}

// What bv_engine_text_parse_bgzf and bv_engine_text_parse_bgzf_region (include/basevar_amd_region.h) share: the runs checked,
// inflated back to back and their line breaks counted per tile (bgzf_runs_begin), and the rows of a line index parsed
// (bgzf_rows_parse).  Between the two each takes its rows its own way.
namespace {
struct BgzfRuns {
    uint32_t F = 0, n_samples = 0, tiles = 0, Pmax = 0;
    std::vector<BvBgzfMember> hd;
    std::vector<LineFile> fl;
    BvTextState *t = nullptr;
    hipStream_t st = nullptr;
    LineFile *d_fl = nullptr;
    uint32_t *d_cnt = nullptr, *d_npos = nullptr;
    size_t lines_end = 0;  // bytes of d_lines that the line index takes; a caller's own arrays lie behind them
    const char *text = nullptr;
    // inflated offset x of file f's run -> (member, offset)
    void cursor_at(const bv_bgzf_rows *rows, bv_bgzf_cursor *cursor, uint32_t f, uint64_t x) const {
        uint32_t k = rows->file_member[f];
        const uint32_t k1 = rows->file_member[f + 1];
        uint64_t base = 0;
        while (k < k1 && base + hd[k].isize <= x) base += hd[k++].isize;
        cursor[f].member = k - rows->file_member[f];
        cursor[f].offset = k < k1 ? (uint32_t)(x - base) : 0u;
    }
};

// r.tiles == 0 afterwards: no text behind the skips, nothing was launched.  `extra`: bytes of d_lines behind the line index
int bgzf_runs_begin(bv_engine *e, const char *who, const bv_bgzf_rows *rows, const uint8_t *group_id, uint32_t n_groups, uint32_t *n_positions,
                    bv_bgzf_cursor *cursor, void *stream_, size_t extra, BgzfRuns &r) {
    if (!rows->member_off || !rows->file_member || !rows->file_samples || !rows->skip_bytes || !rows->skip_lines)
        return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null member_off/file_member/file_samples/skip_bytes/skip_lines");
    if (rows->reserved_ || rows->at_end > 1u) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": reserved_ must be zero, at_end 0 or 1");
    if (rows->n_files == 0 || rows->max_positions == 0)
        return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": n_files and max_positions must be > 0");
    const uint32_t F = r.F = rows->n_files;
    uint64_t n_samples = 0;
    if (rows->file_member[0] != 0) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": file_member[0] must be 0");
    for (uint32_t f = 0; f < F; ++f)
        if (rows->file_member[f + 1] < rows->file_member[f]) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": file_member out of order");
    if (!rows->data && rows->file_member[F]) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null data");
    int rc = text_check_samples_groups(e, who, rows->file_samples, F, group_id, n_groups, &n_samples);
    if (rc != BV_OK) return rc;
    *n_positions = 0;
    bv_bgzf_members mb{rows->data, rows->member_off, rows->data_bytes, rows->file_member[F], 0};
    std::vector<BvBgzfMember> &hd = r.hd;
    std::vector<uint8_t> pre;
    rc = bv_bgzf_headers(e, who, &mb, hd, pre);
    if (rc != BV_OK) return rc;
    BvTextState *t = engine_state(e, e->text);
    t->parsed = false;
    t->bgzf_rows = false;
    t->job.open = false;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    if ((rc = bv_text_tokens_begin(e, 0, F, st)) != BV_OK) return rc;  // (a call that takes no position leaves no token list either)
    // where every member's text goes: file f's members back to back, one spare byte behind each run (16-byte aligned runs)
    const uint32_t M = mb.n_members;
    std::vector<uint64_t> out_pos(M + 1, 0);
    std::vector<LineFile> &fl = r.fl;
    fl.assign(F, LineFile());
    uint64_t at = 0;
    uint32_t tiles = 0;
    for (uint32_t f = 0; f < F; ++f) {
        LineFile &L = fl[f];
        L.base = at;
        for (uint32_t k = rows->file_member[f]; k < rows->file_member[f + 1]; ++k) {
            out_pos[k] = at;
            at += hd[k].isize;
        }
        L.len = at - L.base;
        L.skip = rows->skip_bytes[f]; L.skip_lines = rows->skip_lines[f]; L.reserved_ = 0;
        if (L.skip > L.len)
            return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": skip_bytes of file " + std::to_string(f) + " is beyond its run");
        L.tile_first = tiles;
        L.n_tiles = L.len > L.skip ? (uint32_t)((L.len + rows->at_end - L.skip + kLineTile - 1) / kLineTile) : 0u;
        tiles += L.n_tiles;
        at = (at + 1 + 15) & ~(uint64_t)15;
    }
    out_pos[M] = at;
    BV_HIP(e, hipSetDevice(t->device));
    rc = grow_device(e, &t->d_btext, &t->btext_bytes, up256(at + 16));
    if (rc != BV_OK) return rc;
    std::vector<uint8_t> status(M ? M : 1);
    if (M) {
        rc = bv_bgzf_inflate_placed(e, &mb, hd, pre, out_pos.data(), t->d_btext, status.data(), st);
        if (rc != BV_OK) return rc;
    }
    for (uint32_t f = 0; f < F; ++f)
        for (uint32_t k = rows->file_member[f]; k < rows->file_member[f + 1]; ++k)
            if (status[k] != BV_BGZF_OK)
                return fail(e, BV_ERR_DATA, std::string(who) + ": file " + std::to_string(f) + ", member " + std::to_string(k - rows->file_member[f]) +
                                                          " of its run: BGZF status " + std::to_string(status[k]) +
                                                          (status[k] == BV_BGZF_BAD_HEADER ? " (bad header)" : status[k] == BV_BGZF_BAD_DEFLATE ? " (invalid DEFLATE stream)"
                                                           : status[k] == BV_BGZF_BAD_SIZE ? " (inflated size is not ISIZE)" : " (CRC32 mismatch)"));
    r.n_samples = (uint32_t)n_samples; r.tiles = tiles; r.t = t; r.st = st;
    for (uint32_t f = 0; f < F; ++f) r.cursor_at(rows, cursor, f, fl[f].skip);
    r.Pmax = std::min(rows->max_positions, e->cfg.max_sites);
    if (tiles == 0) return BV_OK;
    // the line index
    const size_t o_cnt = up256(sizeof(LineFile) * F), o_npos = o_cnt + up256(4ull * tiles);
    r.lines_end = o_npos + 256;
    rc = grow_device(e, &t->d_lines, &t->lines_bytes, r.lines_end + extra + (extra ? up256(sizeof(bv_tr_tile) * tiles) : 0));
    if (rc != BV_OK) return rc;
    r.d_fl = reinterpret_cast<LineFile *>(t->d_lines);
    r.d_cnt = reinterpret_cast<uint32_t *>(t->d_lines + o_cnt);
    r.d_npos = reinterpret_cast<uint32_t *>(t->d_lines + o_npos);
    r.text = reinterpret_cast<const char *>(t->d_btext);
    BV_HIP(e, hipMemcpyAsync(r.d_fl, fl.data(), sizeof(LineFile) * F, hipMemcpyHostToDevice, st));
    BV_HIP(e, hipMemcpyAsync(r.d_npos, &r.Pmax, 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bv_text_line_pad_kernel, dim3((F + 63u) / 64u), dim3(64), 0, st, (char *)t->d_btext, (const LineFile *)r.d_fl, F);
    hipLaunchKernelGGL(bv_text_line_count_kernel, dim3(tiles), dim3(64), 0, st, r.text, (const LineFile *)r.d_fl, F, rows->at_end, r.d_cnt);
    hipLaunchKernelGGL(bv_text_line_scan_kernel, dim3(1), dim3(256), 0, st, (const LineFile *)r.d_fl, F, r.d_cnt, r.d_npos);
    BV_HIP(e, hipGetLastError());
    return BV_OK;
}

// the P * F rows of (row_beg, row_end) parsed; last[f] = the end of file f's last row
int bgzf_rows_parse(bv_engine *e, const BgzfRuns &r, uint32_t P, uint64_t *row_beg, uint64_t *row_end, const ParseBufs &pb, const uint8_t *group_id,
                    uint32_t n_groups, uint8_t *row_state, std::vector<uint64_t> &last) {
    const uint32_t F = r.F;
    hipStream_t st = r.st;
    const size_t R = (size_t)P * F;
    TextParseArgs a;
    a.text = r.text; a.row_beg = row_beg; a.row_end = row_end; a.foff = pb.foff; a.fsamp = pb.fsamp; a.chunk_base = 0;
    a.row_first = 0; a.n_rows_chunk = (uint32_t)R; a.n_files = F; a.pitch = pb.pitch;
    a.bs = pb.bs; a.q = pb.q; a.mq = pb.mq; a.st = pb.stp; a.ref = pb.ref; a.rowflag = pb.rowflag; a.rp = pb.rp;
    a.depth = pb.depth; a.pstate = pb.pstate; a.pmax = pb.pmax;
    hipLaunchKernelGGL(bv_text_parse_kernel, dim3((a.n_rows_chunk + 3u) / 4u), dim3(256), 0, st, a);
    BV_HIP(e, hipGetLastError());
    int rc = bv_text_tokens_rows(e, BvTextTokRows{r.text, row_beg, row_end, pb.rowflag, pb.foff, 0, 0, (uint32_t)R, F}, st);
    if (rc != BV_OK) return rc;
    last.resize(F);
    BV_HIP(e, hipMemcpyAsync(last.data(), row_end + (R - F), 8ull * F, hipMemcpyDeviceToHost, st));
    rc = text_parse_finish(e, r.t, P, F, r.n_samples, group_id, n_groups, row_state, st, pb);  // (synchronises: `last` is there)
    if (rc != BV_OK) {
        r.t->parsed = false;
        return rc;
    }
    r.t->bz_row_beg = row_beg; r.t->bz_row_end = row_end; r.t->bz_rowflag = pb.rowflag;
    r.t->bgzf_rows = true;
    return BV_OK;
}
}  // namespace

int bv_engine_text_parse_bgzf(bv_engine *e, const bv_bgzf_rows *rows, const uint8_t *group_id, uint32_t n_groups, uint32_t *n_positions,
                              uint8_t *row_state, bv_bgzf_cursor *cursor, void *stream_) {
    const char *who = "bv_engine_text_parse_bgzf";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, std::string(who) + ": null engine");
    if (!rows || !row_state || !n_positions || !cursor) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null rows/n_positions/row_state/cursor");
    BgzfRuns r;
    int rc = bgzf_runs_begin(e, who, rows, group_id, n_groups, n_positions, cursor, stream_, 0, r);
    if (rc != BV_OK || r.tiles == 0) return rc;  // (no text behind the skips: no position)
    const uint32_t F = r.F;
    hipStream_t st = r.st;
    uint32_t P = 0;
    BV_HIP(e, hipMemcpyAsync(&P, r.d_npos, 4, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    if (P == 0) return BV_OK;
    ParseBufs pb;
    rc = text_parse_begin(e, r.t, P, F, rows->file_samples, r.n_samples, st, &pb);
    if (rc != BV_OK) return rc;
    const size_t R = (size_t)P * F;
    uint64_t *row_beg = pb.d_off, *row_end = pb.d_off + R;
    hipLaunchKernelGGL(bv_text_line_scatter_kernel, dim3(r.tiles), dim3(64), 0, st, r.text, (const LineFile *)r.d_fl, F, rows->at_end, (const uint32_t *)r.d_cnt, P,
                       row_beg, row_end);
    BV_HIP(e, hipGetLastError());
    std::vector<uint64_t> last;
    rc = bgzf_rows_parse(e, r, P, row_beg, row_end, pb, group_id, n_groups, row_state, last);
    if (rc != BV_OK) return rc;
    for (uint32_t f = 0; f < F; ++f) r.cursor_at(rows, cursor, f, std::min(last[f] - r.fl[f].base, r.fl[f].len));
    *n_positions = P;
    return BV_OK;
}

// The rows of a region (bv_text_region_core.h): behind the line index the heads are read and folded, the scatter runs from each
// file's first reached line, POS is held equal across the files, and the rows are parsed as bv_engine_text_parse_bgzf's are.
int bv_engine_text_parse_bgzf_region(bv_engine *e, const bv_bgzf_rows *rows, const bv_text_region *region, const uint8_t *group_id, uint32_t n_groups,
                                     uint32_t *n_positions, uint8_t *row_state, bv_bgzf_cursor *cursor, uint32_t *region_done, void *stream_) {
    const char *who = "bv_engine_text_parse_bgzf_region";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, std::string(who) + ": null engine");
    if (!rows || !row_state || !n_positions || !cursor) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null rows/n_positions/row_state/cursor");
    if (!region || !region_done) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null region/region_done");
    if (!region->name || region->name_len == 0) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": the region needs a name");
    if (region->beg == 0 || region->beg > region->end) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": the region needs 1 <= beg <= end");
    if (region->reserved_) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": the region's reserved_ must be zero");
    *region_done = 0;
    BgzfRuns r;
    const uint32_t F0 = rows->n_files;
    // behind the line index: file results, the scatter's LineFiles, the result and the POS check's word, the name -- and the tile summaries
    const size_t o_file = 0, o_sel = o_file + up256(sizeof(bv_tr_file) * F0), o_res = o_sel + up256(sizeof(LineFile) * F0), o_name = o_res + 256,
                 o_tile = o_name + up256(region->name_len);
    int rc = bgzf_runs_begin(e, who, rows, group_id, n_groups, n_positions, cursor, stream_, o_tile, r);
    if (rc != BV_OK) return rc;
    if (r.tiles == 0) {  // no text behind the skips: no position
        *region_done = rows->at_end;
        return BV_OK;
    }
    const uint32_t F = r.F, tiles = r.tiles;
    BvTextState *t = r.t;
    hipStream_t st = r.st;
    const char *text = r.text;
    uint8_t *mine = t->d_lines + r.lines_end;
    bv_tr_file *d_file = reinterpret_cast<bv_tr_file *>(mine + o_file);
    LineFile *d_sel = reinterpret_cast<LineFile *>(mine + o_sel);
    bv_tr_result *d_res = reinterpret_cast<bv_tr_result *>(mine + o_res);
    uint32_t *d_err = reinterpret_cast<uint32_t *>(d_res + 1);
    char *d_name = reinterpret_cast<char *>(mine + o_name);
    bv_tr_tile *d_tile = reinterpret_cast<bv_tr_tile *>(mine + o_tile);
    BV_HIP(e, hipMemcpyAsync(d_name, region->name, region->name_len, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bv_text_region_head_kernel, dim3(tiles), dim3(64), 0, st, text, (const LineFile *)r.d_fl, F, rows->at_end, (const uint32_t *)r.d_cnt,
                       bv_tr_region{d_name, region->name_len, region->beg, region->end}, d_tile);
    hipLaunchKernelGGL(bv_text_region_combine_kernel, dim3(1), dim3(256), 0, st, (const LineFile *)r.d_fl, F, (const bv_tr_tile *)d_tile, r.Pmax, rows->at_end, d_file,
                       d_sel, d_res);
    BV_HIP(e, hipGetLastError());
    bv_tr_result res;
    std::vector<bv_tr_file> sel(F);
    BV_HIP(e, hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipMemcpyAsync(sel.data(), d_file, sizeof(bv_tr_file) * F, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    if (res.err == BV_TR_ERR_HEAD)
        return fail(e, BV_ERR_DATA, std::string(who) + ": file " + std::to_string(res.err_file) + ", line " + std::to_string(res.err_line) +
                                        " behind its skip: the head is not CHROM, a tab, POS of 1 to 10 digits <= 4294967295, a tab");
    if (res.err == BV_TR_ERR_COUNT)
        return fail(e, BV_ERR_DATA, std::string(who) + ": file " + std::to_string(res.err_file) + ", line " + std::to_string(res.err_line) +
                                        " behind its skip: the file's lines of the region end here, file " + std::to_string(res.err_file2) + " has more");
    const uint32_t P = res.P;
    // the taken rows and one more, whose begin is the cursor
    const size_t R1 = ((size_t)P + 1) * F;
    rc = grow_device(e, &t->d_rrows, &t->rrows_bytes, up256(16 * R1));
    if (rc != BV_OK) return rc;
    uint64_t *row_beg = reinterpret_cast<uint64_t *>(t->d_rrows), *row_end = row_beg + R1;
    const uint32_t none = BV_TR_NONE;
    BV_HIP(e, hipMemcpyAsync(d_err, &none, 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bv_text_line_scatter_kernel, dim3(tiles), dim3(64), 0, st, text, (const LineFile *)d_sel, F, rows->at_end, (const uint32_t *)r.d_cnt, P + 1u,
                       row_beg, row_end);
    if (P && F > 1)
        hipLaunchKernelGGL(bv_text_region_pos_kernel, dim3((uint32_t)(((size_t)P * F + 255) / 256)), dim3(256), 0, st, text, (const uint64_t *)row_beg,
                           (const uint64_t *)row_end, (uint32_t)((size_t)P * F), F, d_err);
    BV_HIP(e, hipGetLastError());
    uint32_t bad = BV_TR_NONE;
    std::vector<uint64_t> next(F);
    BV_HIP(e, hipMemcpyAsync(&bad, d_err, 4, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipMemcpyAsync(next.data(), row_beg + (size_t)P * F, 8ull * F, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    if (bad != BV_TR_NONE)
        return fail(e, BV_ERR_DATA, std::string(who) + ": file " + std::to_string(bad % F) + ", position " + std::to_string(bad / F) + " of the region's rows (line " +
                                        std::to_string(sel[bad % F].first + bad / F) + " behind its skip): POS differs from file 0's");
    // a file without a line stays where it was; every other one goes to its line first + P
    for (uint32_t f = 0; f < F; ++f)
        if (sel[f].n_lines) r.cursor_at(rows, cursor, f, std::min(next[f] - r.fl[f].base, r.fl[f].len));
    *region_done = res.done;
    if (P == 0) return BV_OK;
    ParseBufs pb;
    rc = text_parse_begin(e, t, P, F, rows->file_samples, r.n_samples, st, &pb);
    if (rc != BV_OK) return rc;
    std::vector<uint64_t> last;
    rc = bgzf_rows_parse(e, r, P, row_beg, row_end, pb, group_id, n_groups, row_state, last);
    if (rc != BV_OK) return rc;
    *n_positions = P;
    return BV_OK;
}

// bv_engine_text_rows_fetch, and with `heads` bv_engine_text_heads_fetch (include/basevar_amd_text_tokens.h)
static int text_rows_fetch(bv_engine *e, const char *who, uint32_t heads, uint8_t *buf, uint64_t capacity, uint64_t *row_off, uint64_t *bytes_needed,
                           void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, std::string(who) + ": null engine");
    if (!bytes_needed) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null bytes_needed");
    BvTextState *t = e->text;
    if (!t || !t->bgzf_rows) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": no bv_engine_text_parse_bgzf before it");
    // (the heads leave the marked rows' tokens behind: only where the engine holds them)
    if (heads && !bv_text_tokens_stand(e)) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": the parse did not list the tokens (bv_engine_text_tokens_enable)");
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    BV_HIP(e, hipSetDevice(t->device));
    const uint32_t P = t->n_pos, F = t->n_files;
    const size_t R = (size_t)P * F;
    const uint64_t *row_beg = t->bz_row_beg, *row_end = t->bz_row_end;
    const uint8_t *rowflag = t->bz_rowflag;
    const char *text = reinterpret_cast<const char *>(t->d_btext);
    const size_t o_len = up256(P), o_roff = o_len + up256(4 * R), o_bytes = o_roff + up256(8 * (R + 1));
    int rc = grow_device(e, &t->d_fetch, &t->fetch_bytes, o_bytes);
    if (rc != BV_OK) return rc;
    uint32_t *d_len = reinterpret_cast<uint32_t *>(t->d_fetch + o_len);
    BV_HIP(e, hipMemcpyAsync(t->d_fetch, t->pos_state.data(), P, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bv_text_fetch_len_kernel, dim3((uint32_t)((R + 255) / 256)), dim3(256), 0, st, text, row_beg, row_end, (const uint8_t *)t->d_fetch, rowflag,
                       (uint32_t)R, F, heads, d_len);
    BV_HIP(e, hipGetLastError());
    std::vector<uint32_t> len(R);
    BV_HIP(e, hipMemcpyAsync(len.data(), d_len, 4 * R, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    std::vector<uint64_t> off(R + 1, 0);
    for (size_t r = 0; r < R; ++r) off[r + 1] = off[r] + len[r];
    *bytes_needed = off[R];
    if (capacity < off[R]) return BV_OK;
    if (!row_off || (!buf && off[R])) return fail(e, BV_ERR_INVALID_ARG, std::string(who) + ": null buf/row_off");
    std::memcpy(row_off, off.data(), 8 * (R + 1));
    if (off[R] == 0) return BV_OK;
    // the gathered bytes live behind the offsets; the buffer may move when it grows, so the lengths are copied again after it
    const size_t need = o_bytes + up256(off[R]);
    if (need > t->fetch_bytes) {
        rc = grow_device(e, &t->d_fetch, &t->fetch_bytes, need);
        if (rc != BV_OK) return rc;
        d_len = reinterpret_cast<uint32_t *>(t->d_fetch + o_len);
        BV_HIP(e, hipMemcpyAsync(d_len, len.data(), 4 * R, hipMemcpyHostToDevice, st));
    }
    uint64_t *d_roff = reinterpret_cast<uint64_t *>(t->d_fetch + o_roff);
    BV_HIP(e, hipMemcpyAsync(d_roff, off.data(), 8 * (R + 1), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bv_text_fetch_copy_kernel, dim3((uint32_t)((R + 3) / 4)), dim3(256), 0, st, text, row_beg, (const uint32_t *)d_len, (const uint64_t *)d_roff,
                       (uint32_t)R, t->d_fetch + o_bytes);
    BV_HIP(e, hipGetLastError());
    BV_HIP(e, hipMemcpyAsync(buf, t->d_fetch + o_bytes, off[R], hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    return BV_OK;
}

int bv_engine_text_last_layout(bv_engine *e, uint32_t *layout) {
    if (!e || !layout) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_text_last_layout: null engine/layout");
    if (!e->text || !e->text->sub_rows) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_text_last_layout: no bv_engine_text_submit that called a position");
    *layout = e->text->sub_layout;
    return BV_OK;
}

int bv_engine_text_rows_fetch(bv_engine *e, uint8_t *buf, uint64_t capacity, uint64_t *row_off, uint64_t *bytes_needed, void *stream_) {
    return text_rows_fetch(e, "bv_engine_text_rows_fetch", 0u, buf, capacity, row_off, bytes_needed, stream_);
}

int bv_engine_text_heads_fetch(bv_engine *e, void *buf, uint64_t capacity, uint64_t *row_off, uint64_t *bytes_needed, void *stream_) {
    return text_rows_fetch(e, "bv_engine_text_heads_fetch", 1u, static_cast<uint8_t *>(buf), capacity, row_off, bytes_needed, stream_);
}

}  // extern "C"
