// bv_pileup_text_parts.hip -- batchfile rows over SAMPLE PARTS of piled-up planes (bv_engine_pileup_text_parts,
// include/basevar_amd_pileup_text_parts.h; the contract is INTEGRATION.md section 2o): from one wide pileup, the rows of several
// column ranges of it, each the text of a batchfile of its own.  The bytes: "ROWS OF A PART" in bv_pileup_text_core.h.
// Compiler's resource summary (gfx950): count 66 VGPRs / 46 SGPRs / 5,120 B LDS, scan 18 VGPRs / 20 SGPRs / no LDS, write 66 VGPRs /
// 92 SGPRs / 9,216 B LDS; no scratch, no spilled register.
#include "bv_pileup_text_impl.h"

namespace {

// A part is a tile of its own: its rows are whole-tile rows of the columns [part_first[p], part_first[p + 1]), so one wave handles
// one (part, row, tile OF THE PART) -- a part's tiles are laid out from its first column, 200 samples are one tile wherever they
// start -- and bv_pileup_text_impl.h's list writer runs unchanged on a PtextArgs of the part: n_samples the part's, tokens the part's own
// (the host sorts the rows' tokens by part and rebases their samples; a token in a gap goes nowhere).  What differs is
//   staging  a part starts at any column residue r modulo 16.  A lane takes the aligned 16-byte words that enclose its 16 cells
//            (two of a byte plane, up to four of the rank plane; no misaligned load, none beyond the word that holds the tile's
//            last cell) and shifts them by r cells in registers, so LDS holds the tile from its column 0, as a whole tile's.  Cells of the
//            enclosing words outside the tile are shifted out or lie behind cnt, where nothing looks.
//   depth    the count pass also counts rank != 0 of the tile; the scan sums it per (part, row) beside the list bytes.
// Blocks are part-major, then row, then tile: block b is unit b of tile_sum, and (part, row) x = part * n_rows + row is the row
// of head_off, row_off, row_sum and row_depth, as the text is laid out.  No atomics, no scratch, vector stores only.
struct PartsArgs {
    PtextArgs a;                 // n_samples, n_tiles, tokens, n_tokens: unused here, the kernels fill in the part's
    const uint32_t *part_first;  // [n_parts + 1]
    const uint32_t *tile_base;   // [n_parts + 1]: the tiles of the parts before part p
    const uint64_t *tok_first;   // [n_parts + 1]: part p's tokens are a.tokens [tok_first[p], tok_first[p + 1]), samples rebased
    uint32_t *tile_depth;        // [n_rows x all tiles]
    uint32_t *row_depth;         // [n_parts][n_rows]
    uint32_t n_parts;
};

struct PartOfBlock {
    uint32_t part, k, tile, tiles, cnt, col;  // col: the tile's first column of the planes
};

// (also makes `a` the part's: n_samples, n_tiles, tokens)
__device__ __forceinline__ PartOfBlock part_of_block(const PartsArgs &q, PtextArgs &a) {
    const uint32_t b = blockIdx.x, nr = q.a.n_rows;
    uint32_t lo = 0, hi = q.n_parts;  // the last part whose first block is at or before b
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (nr * q.tile_base[mid] <= b) lo = mid; else hi = mid;
    }
    const uint32_t base = q.tile_base[lo], tiles = q.tile_base[lo + 1u] - base, rest = b - nr * base;
    const uint32_t s0 = q.part_first[lo], n = q.part_first[lo + 1u] - s0, tile = rest % tiles;
    const uint64_t t0 = q.tok_first[lo];
    a.n_samples = n; a.n_tiles = tiles;
    a.tokens = q.a.tokens + t0; a.n_tokens = q.tok_first[lo + 1u] - t0;
    return {lo, rest / tiles, tile, tiles, min(BV_PTEXT_TILE, n - tile * BV_PTEXT_TILE), s0 + tile * BV_PTEXT_TILE};
}

// The four bytes at byte 4 Q + b8 / 8 of the dwords d: a shift of the lane's aligned words by whole cells.  Constant indices
// throughout, so that the words stay in registers
template <uint32_t Q, size_t N>
__device__ __forceinline__ uint32_t shifted_dword(const uint32_t (&d)[N], uint32_t b8) {
    static_assert(Q + 1u < N, "inside the lane's words");
    return (uint32_t)(((((uint64_t)d[Q + 1u]) << 32) | d[Q]) >> b8);
}
template <uint32_t Q, size_t N>
__device__ __forceinline__ uint4 shifted_word(const uint32_t (&d)[N], uint32_t b8) {
    return make_uint4(shifted_dword<Q>(d, b8), shifted_dword<Q + 1u>(d, b8), shifted_dword<Q + 2u>(d, b8), shifted_dword<Q + 3u>(d, b8));
}

// an aligned word, or zeros where the tile has no cell in it
__device__ __forceinline__ uint4 word_if(bool in, const uint4 *p) {
    if (!in) return make_uint4(0, 0, 0, 0);
    return *p;
}

// the lane's 16 cells of a byte plane row whose tile begins r cells behind the aligned `p`
__device__ __forceinline__ uint4 part_load16(const uint8_t *p, uint32_t r, uint32_t cnt, uint32_t lane) {
    const uint32_t end = r + cnt;  // cells of the aligned stream up to the tile's last
    const uint4 *w = reinterpret_cast<const uint4 *>(p) + lane;
    const bool in = 16u * lane < cnt;
    const uint4 w0 = word_if(in, w);
    const uint4 w1 = word_if(in && r != 0u && 16u * (lane + 1u) < end, w + 1);
    const uint32_t d[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    const uint32_t b8 = 8u * (r & 3u);
    switch (r >> 2) {
    case 0: return shifted_word<0>(d, b8);
    case 1: return shifted_word<1>(d, b8);
    case 2: return shifted_word<2>(d, b8);
    default: return shifted_word<3>(d, b8);
    }
}

// the same for the plane of uint16: 32 bytes a lane from up to four aligned words of 8 cells
template <uint32_t Q>
__device__ __forceinline__ void shifted_words2(const uint32_t (&d)[16], uint32_t b8, uint4 *dst) {
    dst[0] = shifted_word<Q>(d, b8);
    dst[1] = shifted_word<Q + 4u>(d, b8);
}
__device__ __forceinline__ void part_load16x2(const uint16_t *p, uint32_t r, uint32_t cnt, uint32_t lane, uint4 *dst) {
    const uint32_t end = r + cnt;
    const uint4 *w = reinterpret_cast<const uint4 *>(p) + 2u * lane;
    const bool in = 16u * lane < cnt;
    const uint4 w0 = word_if(in, w);
    const uint4 w1 = word_if(in && 8u * (2u * lane + 1u) < end, w + 1);
    const uint4 w2 = word_if(in && r != 0u && 8u * (2u * lane + 2u) < end, w + 2);
    const uint4 w3 = word_if(in && r > 8u && 8u * (2u * lane + 3u) < end, w + 3);
    const uint32_t d[16] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
    const uint32_t b8 = 16u * (r & 1u);
    switch (r >> 1) {
    case 0: shifted_words2<0>(d, b8, dst); break;
    case 1: shifted_words2<1>(d, b8, dst); break;
    case 2: shifted_words2<2>(d, b8, dst); break;
    case 3: shifted_words2<3>(d, b8, dst); break;
    case 4: shifted_words2<4>(d, b8, dst); break;
    case 5: shifted_words2<5>(d, b8, dst); break;
    case 6: shifted_words2<6>(d, b8, dst); break;
    default: shifted_words2<7>(d, b8, dst); break;
    }
}

// the part's tile of the four plane rows to LDS, from its column 0; lanes beyond the tile's samples store zeros
__device__ __forceinline__ void part_stage(TileRows *t, const PtextArgs &a, uint32_t k, uint32_t col, uint32_t cnt, uint32_t lane) {
    const uint32_t r = col & 15u;
    const size_t at = (size_t)(a.row0 + k) * a.pitch + (size_t)(col - r);
    reinterpret_cast<uint4 *>(t->cell)[lane] = part_load16(a.cell + at, r, cnt, lane);
    reinterpret_cast<uint4 *>(t->qual)[lane] = part_load16(a.qual + at, r, cnt, lane);
    reinterpret_cast<uint4 *>(t->mapq)[lane] = part_load16(a.mapq + at, r, cnt, lane);
    part_load16x2(a.rank + at, r, cnt, lane, reinterpret_cast<uint4 *>(t->rank) + 2u * lane);
}

__global__ __launch_bounds__(64) void bv_pparts_count_kernel(PartsArgs q) {
    __shared__ __attribute__((aligned(16))) TileRows rows;
    PtextArgs a = q.a;
    const PartOfBlock o = part_of_block(q, a);
    const uint32_t lane = threadIdx.x, pos = a.pos0 + o.k;
    if (o.k >= a.n_rows) return;
    part_stage(&rows, a, o.k, o.col, o.cnt, lane);
    __syncthreads();
    uint32_t m = 0, b = 0, r = 0, d = 0, miss = kNoSample;
    for (uint32_t s = lane; s < o.cnt; s += 64u) {
        const uint32_t rk = rows.rank[s];
        if (rk == 0) { m += 1u; b += 1u; r += 1u; continue; }
        d += 1u;
        m += bv_ptext_digits(rows.mapq[s]);
        r += bv_ptext_digits(rk);
        if (bv_ptext_is_indel(rows.cell[s])) {
            const uint32_t sample = o.tile * BV_PTEXT_TILE + s;  // of the part, as its tokens say
            const uint64_t t = bv_ptext_find(a.tokens, a.n_tokens, pos, sample);
            if (t == a.n_tokens) miss = min(miss, sample);
            else b += a.tokens[t].text_len;
        } else {
            b += 1u;
        }
    }
    m = wave_sum(m); b = wave_sum(b); r = wave_sum(r); d = wave_sum(d);
    miss = wave_min(miss);
    if (lane == 0) {
        a.tile_sum[blockIdx.x] = make_uint4(m, b, r, miss);
        q.tile_depth[blockIdx.x] = d;
    }
}

// one thread a (part, row); row_sum.w is the part's first sample without a token, numbered inside the part
__global__ __launch_bounds__(256) void bv_pparts_scan_kernel(PartsArgs q) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, nr = q.a.n_rows;
    if (x >= q.n_parts * nr) return;
    const uint32_t p = x / nr, k = x - p * nr, base = q.tile_base[p], tiles = q.tile_base[p + 1u] - base;
    const size_t u0 = (size_t)nr * base + (size_t)k * tiles;
    uint4 *ts = q.a.tile_sum + u0;
    uint4 run = make_uint4(0, 0, 0, kNoSample);
    uint32_t depth = 0;
    for (uint32_t t = 0; t < tiles; ++t) {
        const uint4 v = ts[t];
        ts[t] = make_uint4(run.x, run.y, run.z, v.w);
        run.x += v.x; run.y += v.y; run.z += v.z; run.w = min(run.w, v.w);
        depth += q.tile_depth[u0 + t];
    }
    q.a.row_sum[x] = run;
    q.row_depth[x] = depth;
}

__global__ __launch_bounds__(64) void bv_pparts_write_kernel(PartsArgs q) {
    __shared__ __attribute__((aligned(16))) TileRows rows;
    __shared__ __attribute__((aligned(16))) uint8_t image[kImage];
    PtextArgs a = q.a;
    const PartOfBlock o = part_of_block(q, a);
    const uint32_t lane = threadIdx.x, n = a.n_samples, pos = a.pos0 + o.k, tile = o.tile, cnt = o.cnt;
    if (o.k >= a.n_rows) return;
    part_stage(&rows, a, o.k, o.col, cnt, lane);
    const size_t x = (size_t)o.part * a.n_rows + o.k;
    const uint64_t head_at = a.head_off[x], head_bytes = a.head_off[x + 1] - head_at, row_at = a.row_off[x];
    const uint4 before = a.tile_sum[blockIdx.x], row = a.row_sum[x];
    const uint4 next = tile + 1u < o.tiles ? a.tile_sum[blockIdx.x + 1u] : row;
    __syncthreads();
    if (tile == 0) head_copy(a.text + row_at, a.head + head_at, head_bytes, lane);
    const uint64_t first = (uint64_t)tile * BV_PTEXT_TILE;
    const uint64_t at_m = row_at + head_bytes, at_b = at_m + row.x + n, at_q = at_b + row.y + n, at_r = at_q + 2ull * n, at_s = at_r + row.z + n;
    write_list<0>(a, rows, image, at_m + before.x + first, (uint64_t)(next.x - before.x) + cnt, tile, cnt, pos, lane);
    write_list<1>(a, rows, image, at_b + before.y + first, (uint64_t)(next.y - before.y) + cnt, tile, cnt, pos, lane);
    write_list<2>(a, rows, image, at_q + 2ull * first, 2ull * cnt, tile, cnt, pos, lane);
    write_list<3>(a, rows, image, at_r + before.z + first, (uint64_t)(next.z - before.z) + cnt, tile, cnt, pos, lane);
    write_list<4>(a, rows, image, at_s + 2ull * first, 2ull * cnt, tile, cnt, pos, lane);
}


// bv_engine_pileup_text_parts behind its checks.  part_first: host [n_parts + 1]
int ptext_format_parts(bv_engine *e, BvPtextState *t, const bv_pileup_text *in, const uint32_t *part_first, uint32_t n_parts, const TileView &v,
                       const BvPileupView &pv, uint64_t *row_off, hipStream_t st) {
    const std::string who = "bv_engine_pileup_text_parts: ";
    const uint32_t n = in->n_rows, pos0 = v.beg + in->first_row;
    const size_t Q = (size_t)n_parts * n;  // (part, row)s
    BV_HIP(e, hipSetDevice(t->text.device));
    std::vector<uint32_t> tile_base(n_parts + 1u, 0);
    for (uint32_t p = 0; p < n_parts; ++p) tile_base[p + 1u] = tile_base[p] + ptext_tiles_of(part_first[p + 1u] - part_first[p]);
    const size_t U = (size_t)n * tile_base[n_parts];  // (part, row, tile)s: one workgroup each
    // the tokens of the rows, [t_lo, t_hi) by position, go up sorted by part: each part's ascending by (pos, sample) with the
    // sample numbered inside the part, as a tile of the part's columns alone would have them; a gap's tokens stay behind
    const BvPtextToken *t_lo = std::lower_bound(v.tokens, v.tokens + v.n_tokens, pos0, [](const BvPtextToken &x, uint32_t p) { return x.pos < p; });
    const BvPtextToken *t_hi = std::lower_bound(t_lo, v.tokens + v.n_tokens, (uint64_t)pos0 + n, [](const BvPtextToken &x, uint64_t p) { return x.pos < p; });
    auto part_of = [&](uint32_t sample) -> uint32_t {  // n_parts: in a gap
        const uint32_t p = (uint32_t)(std::upper_bound(part_first, part_first + n_parts + 1u, sample) - part_first);
        return p == 0 || p > n_parts ? n_parts : p - 1u;
    };
    std::vector<uint64_t> tok_first(n_parts + 2u, 0);
    for (const BvPtextToken *k = t_lo; k < t_hi; ++k) tok_first[part_of(k->sample) + 1u] += 1;
    for (uint32_t p = 0; p <= n_parts; ++p) tok_first[p + 1u] += tok_first[p];
    const uint64_t nt = tok_first[n_parts];
    uint64_t tok_bytes = 0, text_lo = ~0ull, text_hi = 0;
    const size_t o_toktext = up16(sizeof(BvPtextToken) * nt);
    std::vector<uint8_t> h_tok(o_toktext, 0);
    {
        BvPtextToken *out = reinterpret_cast<BvPtextToken *>(h_tok.data());
        std::vector<uint64_t> fill(tok_first.begin(), tok_first.end() - 1);
        for (const BvPtextToken *k = t_lo; k < t_hi; ++k) {
            const uint32_t p = part_of(k->sample);
            if (p == n_parts) continue;
            BvPtextToken &x = out[fill[p]++];
            x = *k;
            x.sample -= part_first[p];
            tok_bytes += k->text_len;
            text_lo = std::min(text_lo, k->text_off);
            text_hi = std::max(text_hi, k->text_off + k->text_len);
        }
    }
    if (nt == 0) text_lo = text_hi = 0;
    if (tok_bytes >= (1ull << 31)) return fail(e, BV_ERR_TOO_LARGE, who + "the token text of the rows reaches 2^31 bytes: format fewer rows a call");
    const size_t up_text = v.explicit_tile ? (size_t)(text_hi - text_lo) : 0;
    // d_sum: tile_sum [U], row_sum [Q], row_depth [Q], the reference's bytes [n] -- these three come back -- then tile_depth [U],
    // part_first, tile_base u32 [n_parts + 1] each, tok_first u64 [n_parts + 1]
    const size_t o_rsum = 16ull * U, o_depth = o_rsum + 16ull * Q, o_ref = o_depth + 4ull * Q, o_tdepth = up16(o_ref + n), o_pfirst = o_tdepth + up16(4ull * U),
                 o_tbase = o_pfirst + up16(4ull * (n_parts + 1u)), o_tfirst = o_tbase + up16(4ull * (n_parts + 1u)), sum_bytes = o_tfirst + 8ull * (n_parts + 1u);
    int rc = grow_device(e, &t->d_tok, &t->tok_cap, up256(o_toktext + up_text + 16));
    if (rc == BV_OK) rc = grow_device(e, &t->d_sum, &t->sum_cap, up256(sum_bytes));
    if (rc != BV_OK) return rc;
    if (nt) {
        if (v.explicit_tile) {  // its text, the rows' part of it, goes up behind the tokens
            BvPtextToken *k = reinterpret_cast<BvPtextToken *>(h_tok.data());
            for (uint64_t i = 0; i < nt; ++i) k[i].text_off -= text_lo;
            h_tok.resize(o_toktext + up_text);
            if (up_text) std::memcpy(h_tok.data() + o_toktext, v.h_text + text_lo, up_text);
        }
        BV_HIP(e, hipMemcpyAsync(t->d_tok, h_tok.data(), h_tok.size(), hipMemcpyHostToDevice, st));
    }
    BV_HIP(e, hipMemcpyAsync(t->d_sum + o_pfirst, part_first, 4ull * (n_parts + 1u), hipMemcpyHostToDevice, st));
    BV_HIP(e, hipMemcpyAsync(t->d_sum + o_tbase, tile_base.data(), 4ull * (n_parts + 1u), hipMemcpyHostToDevice, st));
    BV_HIP(e, hipMemcpyAsync(t->d_sum + o_tfirst, tok_first.data(), 8ull * (n_parts + 1u), hipMemcpyHostToDevice, st));
    PartsArgs q;
    PtextArgs &a = q.a;
    std::vector<uint8_t> up;
    PtextPlanes pl;
    rc = ptext_planes(e, t, in, v, st, up, pl);
    if (rc != BV_OK) return rc;
    a.cell = pl.cell; a.qual = pl.qual; a.mapq = pl.mapq; a.rank = pl.rank; a.pitch = pl.pitch; a.row0 = pl.row0;
    a.tokens = reinterpret_cast<const BvPtextToken *>(t->d_tok); a.n_tokens = nt;
    a.tok_text = v.explicit_tile ? t->d_tok + o_toktext : v.d_text;
    a.head = nullptr; a.head_off = nullptr; a.row_off = nullptr;
    a.tile_sum = reinterpret_cast<uint4 *>(t->d_sum); a.row_sum = reinterpret_cast<uint4 *>(t->d_sum + o_rsum);
    a.text = nullptr;
    a.pos0 = pos0; a.n_rows = n; a.n_samples = v.n_samples; a.n_tiles = tile_base[n_parts];
    q.part_first = reinterpret_cast<const uint32_t *>(t->d_sum + o_pfirst);
    q.tile_base = reinterpret_cast<const uint32_t *>(t->d_sum + o_tbase);
    q.tok_first = reinterpret_cast<const uint64_t *>(t->d_sum + o_tfirst);
    q.tile_depth = reinterpret_cast<uint32_t *>(t->d_sum + o_tdepth);
    q.row_depth = reinterpret_cast<uint32_t *>(t->d_sum + o_depth);
    q.n_parts = n_parts;
    hipLaunchKernelGGL(bv_pparts_count_kernel, dim3((uint32_t)U), dim3(64), 0, st, q);
    BV_HIP(e, hipGetLastError());
    hipLaunchKernelGGL(bv_pparts_scan_kernel, dim3((uint32_t)((Q + 255u) / 256u)), dim3(256), 0, st, q);
    BV_HIP(e, hipGetLastError());
    BV_HIP(e, hipMemcpyAsync(t->d_sum + o_ref, pv.d_ref + (pos0 - 1u), n, hipMemcpyDeviceToDevice, st));
    std::vector<uint8_t> back(o_ref + n - o_rsum);
    BV_HIP(e, hipMemcpyAsync(back.data(), t->d_sum + o_rsum, back.size(), hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    const uint32_t *sums = reinterpret_cast<const uint32_t *>(back.data());
    const uint32_t *depth = reinterpret_cast<const uint32_t *>(back.data() + (o_depth - o_rsum));
    const uint8_t *ref = back.data() + (o_ref - o_rsum);
    std::vector<uint64_t> off(2ull * (Q + 1), 0);  // head_off, then row_off
    std::string heads;
    uint8_t hb[256 + 40];
    for (uint32_t p = 0; p < n_parts; ++p) {
        const uint32_t N = part_first[p + 1u] - part_first[p];
        for (uint32_t k = 0; k < n; ++k) {
            const size_t x = (size_t)p * n + k;
            const uint32_t m = sums[4u * x], b = sums[4u * x + 1u], r = sums[4u * x + 2u], miss = sums[4u * x + 3u];
            if (miss != kNoSample)
                return fail(e, BV_ERR_DATA, who + "the indel cell at pos " + std::to_string(pos0 + k) + ", sample " + std::to_string((uint64_t)part_first[p] + miss) + " has no token");
            if (depth[x] > N) return fail(e, BV_ERR_HIP, who + "row " + std::to_string(k) + " of part " + std::to_string(p) + " came back with a depth beyond its samples");
            const uint64_t hl = bv_ptext_head(in->chrom, in->chrom_len, pos0 + k, ref[k], depth[x], hb);
            heads.append(reinterpret_cast<const char *>(hb), hl);
            off[x + 1] = off[x] + hl;
            off[Q + 1 + x + 1] = off[Q + 1 + x] + hl + (uint64_t)m + b + r + 7ull * N;
        }
    }
    const uint64_t total = off[2ull * Q + 1];
    const size_t o_heads = 16ull * (Q + 1);
    rc = device_text_reserve(e, t->text, total);
    if (rc == BV_OK) rc = grow_device(e, &t->d_head, &t->head_cap, up256(o_heads + heads.size()));
    if (rc != BV_OK) return rc;
    BV_HIP(e, hipMemcpyAsync(t->d_head, off.data(), o_heads, hipMemcpyHostToDevice, st));
    BV_HIP(e, hipMemcpyAsync(t->d_head + o_heads, heads.data(), heads.size(), hipMemcpyHostToDevice, st));
    a.head_off = reinterpret_cast<const uint64_t *>(t->d_head); a.row_off = a.head_off + (Q + 1);
    a.head = t->d_head + o_heads;
    a.text = t->text.d_text;
    hipLaunchKernelGGL(bv_pparts_write_kernel, dim3((uint32_t)U), dim3(64), 0, st, q);
    BV_HIP(e, hipGetLastError());
    BV_HIP(e, hipStreamSynchronize(st));
    std::memcpy(row_off, off.data() + (Q + 1), 8ull * (Q + 1));
    device_text_done(t->text, total);
    return BV_OK;
}


}  // namespace

extern "C" {

int bv_engine_pileup_text_parts(bv_engine *e, const bv_pileup_text_parts *in, uint64_t *row_off, void *stream_) {
    const std::string who = "bv_engine_pileup_text_parts: ";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    if (e->ptext) e->ptext->text.formatted = false;  // (as above)
    if (!in || !in->rows || !row_off) return fail(e, BV_ERR_INVALID_ARG, who + "null in/rows/row_off");
    if (in->reserved_) return fail(e, BV_ERR_INVALID_ARG, who + "reserved_ must be zero");
    if (!in->part_first || in->n_parts == 0) return fail(e, BV_ERR_INVALID_ARG, who + "part_first must name at least one part");
    BvPileupView pv;
    TileView v;
    if (const int rc = ptext_check(e, who, in->rows, pv, v); rc != BV_OK) return rc;
    uint64_t tiles = 0;
    for (uint32_t p = 0; p < in->n_parts; ++p) {
        if (in->part_first[p] >= in->part_first[p + 1u])
            return fail(e, BV_ERR_INVALID_ARG, who + "part_first must be strictly ascending: part " + std::to_string(p) + " is empty or descends");
        tiles += ptext_tiles_of(in->part_first[p + 1u] - in->part_first[p]);
    }
    if (in->part_first[in->n_parts] > v.n_samples)
        return fail(e, BV_ERR_INVALID_ARG, who + "the parts end at sample " + std::to_string(in->part_first[in->n_parts]) + ", beyond the tile's " + std::to_string(v.n_samples));
    // one workgroup per (part, row, tile of the part)
    if (v.n_samples >= (1u << 28) || (uint64_t)in->rows->n_rows * tiles >= (1ull << 26))
        return fail(e, BV_ERR_TOO_LARGE, who + "n_rows x the tiles of all parts reaches 2^26: format fewer rows or parts a call");
    BvPtextState *t = text_state(e, e->ptext);
    if (in->rows->n_rows == 0) return device_text_empty(t->text, row_off);
    return ptext_format_parts(e, t, in->rows, in->part_first, in->n_parts, v, pv, row_off, stream_ ? (hipStream_t)stream_ : e->stream);
}

}  // extern "C"
