// bv_pileup_text.hip -- batchfile rows written on the device from piled-up planes (bv_engine_pileup_text,
// include/basevar_amd_pileup_text.h; the contract is INTEGRATION.md section 2j).  The bytes are defined at the head of
// bv_pileup_text_core.h, which a CPU harness compiles too; this file is their schedule.
//
// A row is its head (CHROM, pos, REF, Depth: host text, uploaded) and five lists -- M B Q R S -- of one token per sample.  Seen from
// a sample, each list takes its token and one more byte (the ' ' behind it; behind the last sample the list's '\t' or '\n'), so a
// sample's bytes land in FIVE places of the line.  Rows are cut into tiles of BV_PTEXT_TILE samples; one wave handles one
// (row, tile):
//   count  the tile's token bytes of M, B and R (Q and S are one byte a sample), a wave reduction each, and the first sample whose
//          indel cell has no token: nothing is written for such rows, the call refuses them.
//   scan   one thread a row: the tile sums become the tiles' prefixes inside each list, their totals the row's.  The row lengths
//          and row_off are then summed on the HOST, which waits for the counts in any case to size the text buffer; it formats
//          the heads meanwhile (they need the depths and n_rows bytes of the reference).
//   write  the tile's four plane rows go to LDS with 16-byte loads; then list by list, 64 samples a step: a wave prefix sum of
//          the token lengths gives lane l its token's place in an LDS image of the tile's piece of the list, which is laid out
//          as the text is modulo 16 (bv_text_image.h).  A step without a claimed cell (a 64-bit ballot) skips the prefix sum: its
//          tokens are the 2-byte placeholders at 2 l.  Neighbouring tiles, lists and rows share 16-byte words, and every byte of
//          the text has exactly one writer.  The image has kImage bytes: where a list's piece is longer -- ranks of five digits,
//          indel tokens of any length -- the whole words are stored, the rest moves to the image's front and the list goes on; a
//          step whose tokens exceed the image goes token by token, the wave across a token's bytes.  Tile 0 copies the head.
// No atomics, no scratch, vector stores only.  Cells at pitch positions at or beyond n_samples are loaded with their 16-byte
// word and never looked at.  The kernels' arguments, the tile's rows in LDS and the list writer are bv_pileup_text_impl.h's, which
// bv_pileup_text_parts.hip (rows over sample parts of a tile) includes too.
#include "bv_pileup_text_impl.h"

static_assert(BV_PTEXT_CELL_NOCALL == BV_CELL_NOCALL && BV_PTEXT_CELL_REV == BV_CELL_REV, "bv_pileup_text_core.h restates the cell bits");
static_assert(sizeof(BvPtextToken) == sizeof(bv_pileup_token) && sizeof(bv_pileup_token) == 24 && sizeof(BvPileupToken) == 24, "one token layout");

namespace {

__global__ __launch_bounds__(64) void bv_ptext_count_kernel(PtextArgs a) {
    __shared__ __attribute__((aligned(16))) TileRows rows;
    const auto [k, tile, cnt] = tile_of_block(a.n_tiles, a.n_samples, BV_PTEXT_TILE);
    const uint32_t lane = threadIdx.x, pos = a.pos0 + k;
    if (k >= a.n_rows) return;
    tile_stage(&rows, a, k, tile, cnt, lane);
    __syncthreads();
    uint32_t m = 0, b = 0, r = 0, miss = kNoSample;
    for (uint32_t s = lane; s < cnt; s += 64u) {
        const uint32_t rk = rows.rank[s];
        if (rk == 0) { m += 1u; b += 1u; r += 1u; continue; }
        m += bv_ptext_digits(rows.mapq[s]);
        r += bv_ptext_digits(rk);
        if (bv_ptext_is_indel(rows.cell[s])) {
            const uint32_t sample = tile * BV_PTEXT_TILE + s;
            const uint64_t t = bv_ptext_find(a.tokens, a.n_tokens, pos, sample);
            if (t == a.n_tokens) miss = min(miss, sample);
            else b += a.tokens[t].text_len;
        } else {
            b += 1u;
        }
    }
    m = wave_sum(m); b = wave_sum(b); r = wave_sum(r);
    miss = wave_min(miss);
    if (lane == 0) a.tile_sum[(size_t)k * a.n_tiles + tile] = make_uint4(m, b, r, miss);
}

__global__ __launch_bounds__(256) void bv_ptext_scan_kernel(PtextArgs a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.n_rows) return;
    uint4 *ts = a.tile_sum + (size_t)k * a.n_tiles;
    uint4 run = make_uint4(0, 0, 0, kNoSample);
    for (uint32_t t = 0; t < a.n_tiles; ++t) {
        const uint4 v = ts[t];
        ts[t] = make_uint4(run.x, run.y, run.z, v.w);
        run.x += v.x; run.y += v.y; run.z += v.z; run.w = min(run.w, v.w);
    }
    a.row_sum[k] = run;
}

__global__ __launch_bounds__(64) void bv_ptext_write_kernel(PtextArgs a) {
    __shared__ __attribute__((aligned(16))) TileRows rows;
    __shared__ __attribute__((aligned(16))) uint8_t image[kImage];
    const auto [k, tile, cnt] = tile_of_block(a.n_tiles, a.n_samples, BV_PTEXT_TILE);
    const uint32_t lane = threadIdx.x, n = a.n_samples, pos = a.pos0 + k;
    if (k >= a.n_rows) return;
    tile_stage(&rows, a, k, tile, cnt, lane);
    const uint64_t head_at = a.head_off[k], head_bytes = a.head_off[k + 1] - head_at, row_at = a.row_off[k];
    const uint4 before = a.tile_sum[(size_t)k * a.n_tiles + tile], row = a.row_sum[k];
    const uint4 next = tile + 1u < a.n_tiles ? a.tile_sum[(size_t)k * a.n_tiles + tile + 1u] : row;
    __syncthreads();
    if (tile == 0) head_copy(a.text + row_at, a.head + head_at, head_bytes, lane);
    // where the five lists of the row begin, and the tile's piece of each: the samples before it took their tokens and one byte each
    const uint64_t first = (uint64_t)tile * BV_PTEXT_TILE;
    const uint64_t at_m = row_at + head_bytes, at_b = at_m + row.x + n, at_q = at_b + row.y + n, at_r = at_q + 2ull * n, at_s = at_r + row.z + n;
    write_list<0>(a, rows, image, at_m + before.x + first, (uint64_t)(next.x - before.x) + cnt, tile, cnt, pos, lane);
    write_list<1>(a, rows, image, at_b + before.y + first, (uint64_t)(next.y - before.y) + cnt, tile, cnt, pos, lane);
    write_list<2>(a, rows, image, at_q + 2ull * first, 2ull * cnt, tile, cnt, pos, lane);
    write_list<3>(a, rows, image, at_r + before.z + first, (uint64_t)(next.z - before.z) + cnt, tile, cnt, pos, lane);
    write_list<4>(a, rows, image, at_s + 2ull * first, 2ull * cnt, tile, cnt, pos, lane);
}

}  // namespace

void bv_ptext_state_free(BvPtextState *t) {
    if (!t) return;
    (void)hipSetDevice(t->text.device);
    for (uint8_t *b : {t->text.d_text, t->d_tok, t->d_head, t->d_sum, t->d_rows})
        if (b) (void)hipFree(b);
    delete t;
}

namespace bv_impl {

int ptext_planes(bv_engine *e, BvPtextState *t, const bv_pileup_text *in, const TileView &v, hipStream_t st, std::vector<uint8_t> &up, PtextPlanes &a) {
    const uint32_t n = in->n_rows, N = v.n_samples;
    a.cell = v.cell; a.qual = v.qual; a.mapq = v.mapq; a.rank = v.rank; a.pitch = v.pitch;
    a.row0 = in->first_row;
    if (!v.explicit_tile) return BV_OK;
    const size_t P = up16(N), plane = (size_t)n * P;
    const int rc = grow_device(e, &t->d_rows, &t->rows_cap, up256(5 * plane));
    if (rc != BV_OK) return rc;
    uint16_t *d_rank = reinterpret_cast<uint16_t *>(t->d_rows + 3 * plane);
    const size_t r0 = (size_t)in->first_row * v.pitch;
    if (v.host_planes) {
        up.assign(5 * plane, 0);
        for (uint32_t k = 0; k < n; ++k) {
            std::memcpy(&up[(size_t)k * P], v.cell + r0 + (size_t)k * v.pitch, N);
            std::memcpy(&up[plane + (size_t)k * P], v.qual + r0 + (size_t)k * v.pitch, N);
            std::memcpy(&up[2 * plane + (size_t)k * P], v.mapq + r0 + (size_t)k * v.pitch, N);
            std::memcpy(&up[3 * plane + 2 * (size_t)k * P], v.rank + r0 + (size_t)k * v.pitch, 2ull * N);
        }
        BV_HIP(e, hipMemcpyAsync(t->d_rows, up.data(), 5 * plane, hipMemcpyHostToDevice, st));
    } else {
        BV_HIP(e, hipMemsetAsync(t->d_rows, 0, 5 * plane, st));
        BV_HIP(e, hipMemcpy2DAsync(t->d_rows, P, v.cell + r0, v.pitch, N, n, hipMemcpyDeviceToDevice, st));
        BV_HIP(e, hipMemcpy2DAsync(t->d_rows + plane, P, v.qual + r0, v.pitch, N, n, hipMemcpyDeviceToDevice, st));
        BV_HIP(e, hipMemcpy2DAsync(t->d_rows + 2 * plane, P, v.mapq + r0, v.pitch, N, n, hipMemcpyDeviceToDevice, st));
        BV_HIP(e, hipMemcpy2DAsync(d_rank, 2 * P, v.rank + r0, 2 * v.pitch, 2ull * N, n, hipMemcpyDeviceToDevice, st));
    }
    a.cell = t->d_rows; a.qual = t->d_rows + plane; a.mapq = t->d_rows + 2 * plane; a.rank = d_rank; a.pitch = P;
    a.row0 = 0;
    return BV_OK;
}

// The checks of a bv_pileup_text that bv_engine_pileup_text and bv_engine_pileup_text_parts share, and the tile it names
int ptext_check(bv_engine *e, const std::string &who, const bv_pileup_text *in, BvPileupView &pv, TileView &v) {
    if (in->reserved_) return fail(e, BV_ERR_INVALID_ARG, who + "reserved_ must be zero");
    if (!in->chrom || in->chrom_len < 1u || in->chrom_len > 255u) return fail(e, BV_ERR_INVALID_ARG, who + "chrom must have 1 to 255 bytes");
    for (uint32_t i = 0; i < in->chrom_len; ++i)
        if (in->chrom[i] == '\t' || in->chrom[i] == '\n' || in->chrom[i] == '\r' || in->chrom[i] == '\0')
            return fail(e, BV_ERR_INVALID_ARG, who + "chrom must not hold a tab, a line break or a NUL");
    bv_pileup_view(e->pileup, &pv);
    if (const bv_pileup_tile *T = in->tile) {
        auto misaligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; };
        if (T->mem_kind != BV_MEM_HOST && T->mem_kind != BV_MEM_DEVICE) return fail(e, BV_ERR_INVALID_ARG, who + "mem_kind must be BV_MEM_HOST or BV_MEM_DEVICE");
        if (T->n_samples == 0 || T->pitch < T->n_samples || (T->pitch & 15ull)) return fail(e, BV_ERR_INVALID_ARG, who + "pitch must be >= n_samples >= 1 and a multiple of 16");
        if (!T->cell || !T->qual || !T->mapq || !T->rank) return fail(e, BV_ERR_INVALID_ARG, who + "null plane");
        if (misaligned(T->cell) || misaligned(T->qual) || misaligned(T->mapq) || misaligned(T->rank)) return fail(e, BV_ERR_INVALID_ARG, who + "planes must be 16-byte aligned");
        if (T->beg == 0 || (uint64_t)T->beg + T->rows > (1ull << 32)) return fail(e, BV_ERR_INVALID_ARG, who + "positions beg .. beg + rows - 1 must be 1-based and fit 32 bits");
        if (T->n_tokens && (!T->tokens || (!T->text && T->text_bytes))) return fail(e, BV_ERR_INVALID_ARG, who + "null tokens/text");
        for (uint64_t k = 0; k < T->n_tokens; ++k) {
            const bv_pileup_token &x = T->tokens[k];
            if (k && !(T->tokens[k - 1].pos < x.pos || (T->tokens[k - 1].pos == x.pos && T->tokens[k - 1].sample < x.sample)))
                return fail(e, BV_ERR_INVALID_ARG, who + "tokens must be strictly ascending by (pos, sample): token " + std::to_string(k) + " is not");
            if (x.text_off > T->text_bytes || x.text_len > T->text_bytes - x.text_off)
                return fail(e, BV_ERR_INVALID_ARG, who + "the text of token " + std::to_string(k) + " lies beyond text_bytes");
        }
        v.cell = T->cell; v.qual = T->qual; v.mapq = T->mapq; v.rank = T->rank; v.pitch = T->pitch;
        v.rows = T->rows; v.n_samples = T->n_samples; v.beg = T->beg;
        v.tokens = reinterpret_cast<const BvPtextToken *>(T->tokens); v.n_tokens = T->n_tokens; v.h_text = T->text;
        v.explicit_tile = true; v.host_planes = T->mem_kind == BV_MEM_HOST;
    } else {
        if (!pv.done) return fail(e, BV_ERR_INVALID_ARG, who + "tile == NULL, and no completed bv_engine_pileup on this engine");
        v.cell = pv.cell; v.qual = pv.qual; v.mapq = pv.mapq; v.rank = pv.rank; v.pitch = pv.pitch;
        v.rows = pv.rows; v.n_samples = pv.n_samples; v.beg = pv.beg; v.depth = pv.depth;
        v.tokens = reinterpret_cast<const BvPtextToken *>(pv.tokens); v.n_tokens = pv.n_tokens; v.d_text = pv.d_text;
    }
    if (v.beg == 0) return fail(e, BV_ERR_INVALID_ARG, who + "positions are 1-based: beg must not be 0");
    if ((uint64_t)in->first_row + in->n_rows > v.rows)
        return fail(e, BV_ERR_INVALID_ARG, who + "rows " + std::to_string(in->first_row) + " + " + std::to_string(in->n_rows) + " are beyond the tile's " + std::to_string(v.rows));
    if (!pv.have_ref) return fail(e, BV_ERR_INVALID_ARG, who + "no reference set: bv_engine_pileup_set_reference comes first");
    if (in->n_rows && (uint64_t)v.beg + in->first_row + in->n_rows - 1u > pv.ref_len)
        return fail(e, BV_ERR_INVALID_ARG, who + "the rows end beyond the reference's " + std::to_string(pv.ref_len) + " bases");
    return BV_OK;
}

}  // namespace bv_impl

namespace {

int ptext_format(bv_engine *e, BvPtextState *t, const bv_pileup_text *in, const TileView &v, const BvPileupView &pv, uint64_t *row_off, hipStream_t st) {
    const std::string who = "bv_engine_pileup_text: ";
    const uint32_t n = in->n_rows, N = v.n_samples, n_tiles = (N + BV_PTEXT_TILE - 1u) / BV_PTEXT_TILE, pos0 = v.beg + in->first_row;
    BV_HIP(e, hipSetDevice(t->text.device));
    // the tokens of the rows: [t_lo, t_hi) by position
    const BvPtextToken *t_lo = std::lower_bound(v.tokens, v.tokens + v.n_tokens, pos0, [](const BvPtextToken &x, uint32_t p) { return x.pos < p; });
    const BvPtextToken *t_hi = std::lower_bound(t_lo, v.tokens + v.n_tokens, (uint64_t)pos0 + n, [](const BvPtextToken &x, uint64_t p) { return x.pos < p; });
    const uint64_t nt = (uint64_t)(t_hi - t_lo);
    uint64_t tok_bytes = 0, text_lo = ~0ull, text_hi = 0;
    for (const BvPtextToken *k = t_lo; k < t_hi; ++k) {
        tok_bytes += k->text_len;
        text_lo = std::min(text_lo, k->text_off);
        text_hi = std::max(text_hi, k->text_off + k->text_len);
    }
    if (nt == 0) text_lo = text_hi = 0;
    if (tok_bytes >= (1ull << 31)) return fail(e, BV_ERR_TOO_LARGE, who + "the token text of the rows reaches 2^31 bytes: format fewer rows a call");
    const size_t o_toktext = up16(sizeof(BvPtextToken) * nt), up_text = v.explicit_tile ? (size_t)(text_hi - text_lo) : 0;
    const size_t o_rsum = 16ull * n * n_tiles, o_depth = o_rsum + 16ull * n, o_ref = o_depth + 8ull * n;
    int rc = grow_device(e, &t->d_tok, &t->tok_cap, up256(o_toktext + up_text + 16));
    if (rc == BV_OK) rc = grow_device(e, &t->d_sum, &t->sum_cap, up256(o_ref + n));
    if (rc != BV_OK) return rc;
    std::vector<uint8_t> h_tok(o_toktext + up_text, 0);
    if (nt) {
        std::memcpy(h_tok.data(), t_lo, sizeof(BvPtextToken) * nt);
        if (v.explicit_tile) {  // its text, the rows' part of it, goes up behind the tokens
            BvPtextToken *k = reinterpret_cast<BvPtextToken *>(h_tok.data());
            for (uint64_t i = 0; i < nt; ++i) k[i].text_off -= text_lo;
            if (up_text) std::memcpy(h_tok.data() + o_toktext, v.h_text + text_lo, up_text);
        }
        BV_HIP(e, hipMemcpyAsync(t->d_tok, h_tok.data(), h_tok.size(), hipMemcpyHostToDevice, st));
    }
    PtextArgs a;
    PtextPlanes pl;
    std::vector<uint8_t> up;
    uint32_t *d_depth = reinterpret_cast<uint32_t *>(t->d_sum + o_depth);
    rc = ptext_planes(e, t, in, v, st, up, pl);
    if (rc != BV_OK) return rc;
    a.cell = pl.cell; a.qual = pl.qual; a.mapq = pl.mapq; a.rank = pl.rank; a.pitch = pl.pitch; a.row0 = pl.row0;
    if (v.explicit_tile) BV_HIP(e, bv_pileup_depth_launch(a.rank, a.pitch, n, d_depth, d_depth + n, st));
    a.tokens = reinterpret_cast<const BvPtextToken *>(t->d_tok); a.n_tokens = nt;
    a.tok_text = v.explicit_tile ? t->d_tok + o_toktext : v.d_text;
    a.head = nullptr; a.head_off = nullptr; a.row_off = nullptr;
    a.tile_sum = reinterpret_cast<uint4 *>(t->d_sum); a.row_sum = reinterpret_cast<uint4 *>(t->d_sum + o_rsum);
    a.text = nullptr;
    a.pos0 = pos0; a.n_rows = n; a.n_samples = N; a.n_tiles = n_tiles;
    hipLaunchKernelGGL(bv_ptext_count_kernel, dim3(n * n_tiles), dim3(64), 0, st, a);
    BV_HIP(e, hipGetLastError());
    hipLaunchKernelGGL(bv_ptext_scan_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, a);
    BV_HIP(e, hipGetLastError());
    // the reference's bytes of the rows cross beside the sums: the heads are host text
    BV_HIP(e, hipMemcpyAsync(t->d_sum + o_ref, pv.d_ref + (pos0 - 1u), n, hipMemcpyDeviceToDevice, st));
    std::vector<uint8_t> back(o_ref + n - o_rsum);
    BV_HIP(e, hipMemcpyAsync(back.data(), t->d_sum + o_rsum, back.size(), hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    const uint32_t *sums = reinterpret_cast<const uint32_t *>(back.data());
    const uint32_t *depth = v.depth ? v.depth + in->first_row : reinterpret_cast<const uint32_t *>(back.data() + (o_depth - o_rsum));
    const uint8_t *ref = back.data() + (o_ref - o_rsum);
    std::vector<uint64_t> off(2ull * (n + 1), 0);  // head_off, then row_off
    std::string heads;
    uint8_t hb[256 + 40];
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t m = sums[4u * k], b = sums[4u * k + 1u], r = sums[4u * k + 2u], miss = sums[4u * k + 3u];
        if (miss != kNoSample)
            return fail(e, BV_ERR_DATA, who + "the indel cell at pos " + std::to_string(pos0 + k) + ", sample " + std::to_string(miss) + " has no token");
        if (depth[k] > N) return fail(e, BV_ERR_HIP, who + "row " + std::to_string(k) + " came back with a depth beyond the samples");
        const uint64_t hl = bv_ptext_head(in->chrom, in->chrom_len, pos0 + k, ref[k], depth[k], hb);
        heads.append(reinterpret_cast<const char *>(hb), hl);
        off[k + 1] = off[k] + hl;
        off[n + 1 + k + 1] = off[n + 1 + k] + hl + (uint64_t)m + b + r + 7ull * N;
    }
    const uint64_t total = off[2ull * n + 1];
    const size_t o_heads = 16ull * (n + 1);
    rc = device_text_reserve(e, t->text, total);
    if (rc == BV_OK) rc = grow_device(e, &t->d_head, &t->head_cap, up256(o_heads + heads.size()));
    if (rc != BV_OK) return rc;
    BV_HIP(e, hipMemcpyAsync(t->d_head, off.data(), o_heads, hipMemcpyHostToDevice, st));
    BV_HIP(e, hipMemcpyAsync(t->d_head + o_heads, heads.data(), heads.size(), hipMemcpyHostToDevice, st));
    a.head_off = reinterpret_cast<const uint64_t *>(t->d_head); a.row_off = a.head_off + (n + 1);
    a.head = t->d_head + o_heads;
    a.text = t->text.d_text;
    hipLaunchKernelGGL(bv_ptext_write_kernel, dim3(n * n_tiles), dim3(64), 0, st, a);
    BV_HIP(e, hipGetLastError());
    BV_HIP(e, hipStreamSynchronize(st));
    std::memcpy(row_off, off.data() + (n + 1), 8ull * (n + 1));
    device_text_done(t->text, total);
    return BV_OK;
}

}  // namespace

extern "C" {

uint32_t bv_pileup_text_tile_samples(void) { return BV_PTEXT_TILE; }

int bv_engine_pileup_text(bv_engine *e, const bv_pileup_text *in, uint64_t *row_off, void *stream_) {
    const std::string who = "bv_engine_pileup_text: ";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    // deliberately on entry, not behind the checks as in bv_engine_vcf_format: whatever comes of this call, the last text is gone
    if (e->ptext) e->ptext->text.formatted = false;
    if (!in || !row_off) return fail(e, BV_ERR_INVALID_ARG, who + "null in/row_off");
    BvPileupView pv;
    TileView v;
    if (const int rc = ptext_check(e, who, in, pv, v); rc != BV_OK) return rc;
    // one workgroup per (row, tile): a launch's grid has room for 2^26 of them; the sums of a row are 32-bit
    if (v.n_samples >= (1u << 28) || (uint64_t)in->n_rows * ((v.n_samples + BV_PTEXT_TILE - 1u) / BV_PTEXT_TILE) >= (1ull << 26))
        return fail(e, BV_ERR_TOO_LARGE, who + "n_rows x tiles of a row reaches 2^26: format fewer rows a call");
    BvPtextState *t = text_state(e, e->ptext);
    if (in->n_rows == 0) return device_text_empty(t->text, row_off);
    return ptext_format(e, t, in, v, pv, row_off, stream_ ? (hipStream_t)stream_ : e->stream);
}

int bv_engine_pileup_text_fetch(bv_engine *e, void *dst, uint64_t dst_capacity, int dst_mem_kind, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_pileup_text_fetch: null engine");
    return device_text_fetch(e, "bv_engine_pileup_text_fetch: ", "bv_engine_pileup_text", e->ptext ? &e->ptext->text : nullptr, dst, dst_capacity, dst_mem_kind, stream_);
}

int bv_engine_pileup_text_deflate(bv_engine *e, const uint64_t *block_off, uint32_t n_blocks, int level, uint8_t *dst, uint64_t dst_capacity,
                                  uint64_t *member_off, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_pileup_text_deflate: null engine");
    return device_text_deflate(e, "bv_engine_pileup_text_deflate: ", "bv_engine_pileup_text", e->ptext ? &e->ptext->text : nullptr, block_off, n_blocks, level, dst, dst_capacity,
                               member_off, stream_);
}

}  // extern "C"

