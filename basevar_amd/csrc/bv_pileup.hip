// bv_pileup.hip -- BAM records piled up on the device (bv_engine_pileup, include/basevar_amd_pileup.h; the contract is
// INTEGRATION.md section 2i), and the same from BGZF members that are still compressed (bv_engine_pileup_bgzf,
// include/basevar_amd_pileup_bgzf.h, section 2k): bv_inflate.hip's kernel inflates them back to back, the runs are cut out of
// that.  The result is defined at the head of bv_pileup_core.h, which a CPU harness compiles too; this file is its schedule.  Of that header the kernels compile the record decode, the filter and the helpers; wave_walk below states
// the walk a second time, and tests/test_gpu_pileup.py (BAM corpus) and tests/test_gpu_pileup_raw.py (raw runs, edges) hold it
// to the first byte for byte.
//
// ONE WAVE PER SAMPLE.  A sample's reads are independent of every other sample's, and "the first read wins" is an order inside
// one sample: so a wave walks its sample's runs record by record, in file order, and first-read-wins is program order.
//   pile     the record's header fields, the filters and the CIGAR operations are wave-uniform (every lane decodes the same
//            bytes); the 64 lanes lie across the bases of a match operation, stride 64.  The wave keeps the sample's `seen` bits
//            of the window in LDS, one bit a row (dynamic LDS: 4 bytes per 32 rows, 62,500 bytes for the largest window, so
//            that two workgroups always fit a CU and a small window leaves the CU to as many waves as it takes).  A lane sets its
//            base's bit with an LDS atomic OR -- neighbouring lanes share a word -- and stores the cell's four plane values
//            only where the bit was clear.  No other wave writes that sample's column: no global atomic, and the planes do not
//            depend on scheduling.  It also counts the sample's indel tokens and their bytes.
//   depth    one wave a row: depth[row] = cells of rank != 0, a row reduction (no atomic add), and the row's largest rank.
//   tokens   the host sums the samples' token counts into their places (sample order); the waves of the samples that have
//            tokens walk their records again -- headers and CIGARs only, no base is looked at -- and write {pos, sample,
//            text_off, text_len} and the text.  A claimed indel is found again without the planes' history: the first attempt on
//            a position claimed it, so a cell that holds an indel was claimed by the first indel that tried, and the `seen`
//            bits, set here by indels alone, tell the first.  The host sorts the descriptors by (pos, sample).
//   gather   one workgroup a covered row: the row's four plane rows into a compact slab, ranks tagged on request, ref_base from
//            the uploaded reference.
// No scratch, vector stores only.  Host records cross the link through bv_chunk_stage.h's pinned chunks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/basevar_amd_pileup.h"
#include "../../include/basevar_amd_pileup_bgzf.h"
#include "bv_chunk_stage.h"
#include "bv_inflate_core.h"
#include "bv_pileup_core.h"

using namespace bv_impl;

static_assert(BV_PU_CELL_REV == BV_CELL_REV && BV_PU_CELL_N == BV_CELL_N && BV_PU_CELL_INS == BV_CELL_INS && BV_PU_CELL_DEL == BV_CELL_DEL,
              "bv_pileup_core.h restates the cell codes");
static_assert(sizeof(BvPileupToken) == sizeof(bv_pileup_token) && sizeof(bv_pileup_token) == 24, "one token layout");
static_assert(sizeof(BvPileupSample) == 32, "per-sample outcome");

namespace {

struct PileupArgs {
    BvPileupQuery q;
    const uint8_t *records;    // run r is records[run_at[2 r] .. run_at[2 r + 1]) (of host records: their device copy less run_off[0])
    const uint64_t *run_at;    // [n_runs][2]: where a run begins and ends; runs need not be neighbours (bv_engine_pileup_bgzf)
    const uint32_t *samp_run;  // [n_samples + 1]: the runs of sample s are [samp_run[s], samp_run[s + 1])
    const uint8_t *ref;
    uint8_t *planes;           // cell, qual, mapq (plane_bytes apart) and rank, [rows][pitch] each
    uint64_t plane_bytes, pitch;
    BvPileupSample *per;       // [n_samples]
    const uint64_t *tok_base, *text_base;  // [n_samples] (token pass)
    BvPileupToken *tokens;
    uint8_t *text;
    uint32_t rows;
};

// The kernel's arguments where the hardware put them.  The walk is scalar code throughout -- every lane decodes the same record --
// and its state, the arguments and what the compiler derives from them (64-bit forms of the window's bounds, the planes'
// addresses, multiples of the pitch) do not fit the scalar register file together if all of it is kept for the whole kernel.  So
// what a record needs is read from the argument segment again for every record (scalar loads that hit the constant cache),
// through a pointer the compiler must take as it stands, and lives no longer than that record.
typedef const __attribute__((address_space(4))) PileupArgs *KernArgs;
__device__ __forceinline__ KernArgs kern_args() {
    KernArgs k = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return k;
}

// what the walk of one record reads of the arguments
struct WalkEnv {
    BvPileupQuery q;
    const uint8_t *cell;    // the first plane
    uint64_t pitch;
    const uint8_t *ref;
    BvPileupToken *tokens;  // the sample's
    uint8_t *text;          // the sample's
};

template <bool TOKENS>
__device__ __forceinline__ void walk_env(uint32_t s, WalkEnv *e) {
    KernArgs k = kern_args();
    e->q.tid = k->q.tid; e->q.beg = k->q.beg; e->q.end = k->q.end; e->q.gb = k->q.gb; e->q.ge = k->q.ge; e->q.mapq_thd = k->q.mapq_thd;
    e->q.ref_len = k->q.ref_len;
    e->cell = k->planes; e->pitch = k->pitch;
    e->ref = k->ref;
    e->tokens = TOKENS ? k->tokens + k->tok_base[s] : nullptr;
    e->text = TOKENS ? k->text + k->text_base[s] : nullptr;
}

// (the planes' addresses are formed where they are used: kept across the walk they cost six scalar registers)
__device__ __forceinline__ void store_cell(uint64_t k, uint32_t code, uint32_t qual, uint32_t mapq, uint32_t rank) {
    KernArgs a = kern_args();
    uint8_t *planes = a->planes;
    const uint64_t plane_bytes = a->plane_bytes;
    planes[k] = (uint8_t)code;
    planes[plane_bytes + k] = (uint8_t)qual;
    planes[2u * plane_bytes + k] = (uint8_t)mapq;
    reinterpret_cast<uint16_t *>(planes + 3u * plane_bytes)[k] = (uint16_t)rank;
}

// One record that bv_pileup_filter let through: bv_pileup_walk (bv_pileup_core.h) with the lanes across the bases.
// TOKENS: the second walk, which writes the tokens of the indels that the first one claimed.
template <bool TOKENS>
__device__ __forceinline__ uint32_t wave_walk(const WalkEnv &a, const uint8_t *run, const BvPileupRec &r, uint32_t s, uint32_t lane, uint32_t *seen,
                                              uint32_t &n_tok, uint64_t &text_bytes) {
    const BvPileupQuery &q = a.q;
    const uint32_t strand = (r.flag & 16u) ? BV_PU_CELL_REV : 0u;
    const uint8_t *seq = run + bv_pileup_seq_at(&r), *qual = run + bv_pileup_qual_at(&r);
    uint32_t mean_q = 0;
    if (!TOKENS) {
        unsigned long long sum = 0;
        for (uint32_t i = lane; i < r.l_seq; i += 64u) sum += qual[i];
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
        mean_q = bv_pileup_mean_q(sum, r.l_seq);
    }
    int64_t rpos = r.pos;
    uint32_t qpos = 0;
    for (uint32_t c = 0; c < r.n_cigar; ++c) {
        const uint32_t cig = bv_pileup_u32(run + r.cigar_at + 4ull * c), op = cig & 15u;
        const int64_t len = cig >> 4;
        if (bv_pileup_op_is_match(op)) {
            int64_t i_lo, i_hi;
            const bool ends = bv_pileup_match_range(&q, rpos, len, &i_lo, &i_hi);
            if (!TOKENS) {
                bool over = false, bad = false;
                for (int64_t i0 = i_lo; i0 < i_hi; i0 += 64) {
                    const int64_t i = i0 + lane;
                    if (i >= i_hi) continue;
                    const uint32_t qi = qpos + (uint32_t)i;
                    if (qi >= r.l_seq) { over = true; continue; }
                    const uint32_t code = bv_pileup_base_cell(bv_pileup_nibble(seq, qi));
                    if (code == BV_PU_CELL_BAD) { bad = true; continue; }
                    const int64_t p = rpos + i + 1;
                    if (p < (int64_t)q.beg || p > (int64_t)q.end) continue;
                    const uint64_t row = (uint64_t)(p - q.beg);
                    const uint32_t bit = 1u << (row & 31u);
                    if (atomicOr(&seen[row >> 5], bit) & bit) continue;  // an earlier read holds the cell
                    store_cell(row * a.pitch + s, code | strand, qual[qi], r.mapq, bv_pileup_rank(qi + 1u));
                }
                if (__any(over)) return BV_PILEUP_BAD_QUERY;
                if (__any(bad)) return BV_PILEUP_BAD_BASE;
            }
            if (ends) return BV_PILEUP_OK;
            rpos += len; qpos += (uint32_t)len;
        } else if (op == 1u || op == 2u) {
            const bool ins = op == 1u;
            if ((int64_t)q.ge < rpos + 1) return BV_PILEUP_OK;
            if ((int64_t)q.gb <= rpos + 1 && rpos >= 1 && rpos >= (int64_t)q.beg && rpos <= (int64_t)q.end) {
                const uint64_t row = (uint64_t)(rpos - q.beg);
                const uint32_t bit = 1u << (row & 31u);
                uint32_t old = 0;
                if (lane == 0) old = atomicOr(&seen[row >> 5], bit);
                old = __builtin_amdgcn_readfirstlane(old);  // wave-uniform, and known to be
                if (!(old & bit)) {
                    const uint64_t k = row * a.pitch + s;
                    if (!TOKENS) {
                        if (lane == 0) store_cell(k, (ins ? BV_PU_CELL_INS : BV_PU_CELL_DEL) | strand, mean_q, r.mapq, bv_pileup_rank(qpos + 1u));
                        if ((uint64_t)rpos - 1u >= q.ref_len) return BV_PILEUP_BAD_REF;
                        if (ins && qpos > r.l_seq) return BV_PILEUP_BAD_QUERY;
                        n_tok += 1u;
                        text_bytes += bv_pileup_token_bytes(ins, rpos, qpos, len, r.l_seq, q.ref_len);
                    } else if ((a.cell[k] & BV_PU_CELL_N) && (a.cell[k] & 3u)) {  // the first walk's claim of an indel: this one's
                        const uint64_t bytes = bv_pileup_token_bytes(ins, rpos, qpos, len, r.l_seq, q.ref_len);
                        if (lane == 0) {
                            BvPileupToken t;
                            t.pos = (uint32_t)rpos; t.sample = s; t.text_off = (uint64_t)(a.text - kern_args()->text) + text_bytes; t.text_len = (uint32_t)bytes;
                            t.reserved_ = 0;
                            a.tokens[n_tok] = t;
                        }
                        for (uint64_t j = lane; j < bytes; j += 64u)
                            a.text[text_bytes + j] = j == 0 ? (uint8_t)(ins ? '+' : '-') : j == 1 ? a.ref[rpos - 1]
                                                   : ins ? bv_pileup_letter(bv_pileup_nibble(seq, qpos + (uint32_t)(j - 2u))) : a.ref[(uint64_t)rpos + j - 2u];
                        n_tok += 1u;
                        text_bytes += bytes;
                    }
                }
            }
            if (ins) qpos += (uint32_t)len; else rpos += len;
        } else if (op == 3u) {
            if ((int64_t)q.ge < rpos + 1) return BV_PILEUP_OK;
            rpos += len;
        } else if (op == 4u || op == 6u) {
            if ((int64_t)q.ge < rpos + 1) return BV_PILEUP_OK;
            qpos += (uint32_t)len;
        }
    }
    return BV_PILEUP_OK;
}

// bv_pileup_sample (bv_pileup_core.h) by one wave; grid: one workgroup of one wave a sample
template <bool TOKENS>
__global__ __launch_bounds__(64) void bv_pileup_kernel(PileupArgs) {
    extern __shared__ uint32_t seen[];  // one bit a row of the window
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (TOKENS && kern_args()->per[s].n_tokens == 0) return;
    for (uint32_t w = lane, n = (kern_args()->rows + 31u) / 32u; w < n; w += 64u) seen[w] = 0;
    __syncthreads();
    uint32_t status = BV_PILEUP_OK, fail_run = 0, n_tokens = 0;
    uint64_t fail_at = 0, text_bytes = 0;
    bool live = true;
    const uint32_t run_hi = kern_args()->samp_run[s + 1];
    for (uint32_t r = kern_args()->samp_run[s]; live && r < run_hi; ++r) {
        const uint64_t lo = kern_args()->run_at[2u * r], bytes = kern_args()->run_at[2u * r + 1u] - lo;
        for (uint64_t at = 0; at < bytes;) {
            const uint8_t *run = kern_args()->records + lo;
            BvPileupRec rec;
            uint32_t st = bv_pileup_record(run, bytes, at, &rec);
            if (st == BV_PILEUP_OK) {
                WalkEnv env;
                walk_env<TOKENS>(s, &env);
                const uint32_t what = bv_pileup_filter(&env.q, &rec);
                if (what == BV_PILEUP_BREAK) { live = false; break; }
                if (what == BV_PILEUP_CLAIM) st = wave_walk<TOKENS>(env, run, rec, s, lane, seen, n_tokens, text_bytes);
            }
            if (st != BV_PILEUP_OK) {
                status = st; fail_run = r; fail_at = at;
                live = false;
                break;
            }
            at = rec.next_at;
        }
    }
    if (!TOKENS && lane == 0) {
        BvPileupSample me;
        me.at = fail_at; me.text_bytes = text_bytes; me.status = status; me.run = fail_run; me.n_tokens = n_tokens; me.reserved_ = 0;
        kern_args()->per[s] = me;
    }
}

// depth[row] = cells of rank != 0 and max_rank[row], one wave a row, four rows a workgroup; pitch is a multiple of 16
__global__ __launch_bounds__(256) void bv_pileup_depth_kernel(const uint16_t *rank, uint64_t pitch, uint32_t rows, uint32_t *depth, uint32_t *max_rank) {
    const uint32_t row = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (row >= rows) return;
    const uint4 *p = reinterpret_cast<const uint4 *>(rank + (size_t)row * pitch);
    uint32_t n = 0, mx = 0;
    for (uint64_t j = lane; j < pitch / 8u; j += 64u) {
        const uint4 v = p[j];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t lo = w[i] & 0xffffu, hi = w[i] >> 16;
            n += (lo != 0u) + (hi != 0u);
            mx = max(mx, max(lo, hi));
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        n += __shfl_xor(n, d, 64);
        mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
    }
    if (lane == 0) { depth[row] = n; max_rank[row] = mx; }
}

struct GatherArgs {
    const uint8_t *cell, *qual, *mapq;  // the window's planes
    const uint16_t *rank;
    uint8_t *o_cell, *o_qual, *o_mapq;  // the slab's
    uint16_t *o_rank;
    uint8_t *o_ref;
    const uint32_t *row_of;             // [n]: the window row of slab row k
    const uint8_t *ref;
    uint64_t ref_len, pitch;
    uint32_t beg, tagged;
};

// slab row k = window row row_of[k]; 16 cells a thread and step
__global__ __launch_bounds__(256) void bv_pileup_gather_kernel(GatherArgs a) {
    const uint32_t k = blockIdx.x, row = a.row_of[k];
    const size_t src = (size_t)row * a.pitch, dst = (size_t)k * a.pitch;
    for (uint64_t j = threadIdx.x; j < a.pitch / 16u; j += 256u) {
        const uint4 c = reinterpret_cast<const uint4 *>(a.cell + src)[j];
        reinterpret_cast<uint4 *>(a.o_cell + dst)[j] = c;
        reinterpret_cast<uint4 *>(a.o_qual + dst)[j] = reinterpret_cast<const uint4 *>(a.qual + src)[j];
        reinterpret_cast<uint4 *>(a.o_mapq + dst)[j] = reinterpret_cast<const uint4 *>(a.mapq + src)[j];
        const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint4 rk = reinterpret_cast<const uint4 *>(a.rank + src)[2u * j + h];
            uint32_t w[4] = {rk.x, rk.y, rk.z, rk.w};
            if (a.tagged) {
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) {  // word i holds the ranks of cells 8 h + 2 i and + 1
                    const uint32_t c0 = (cw[2u * h + i / 2u] >> (16u * (i & 1u))) & 0xffu, c1 = (cw[2u * h + i / 2u] >> (16u * (i & 1u) + 8u)) & 0xffu;
                    w[i] = (uint32_t)BV_RPR_TAGGED(c0, w[i] & 0xffffu) | ((uint32_t)BV_RPR_TAGGED(c1, w[i] >> 16) << 16);
                }
            }
            reinterpret_cast<uint4 *>(a.o_rank + dst)[2u * j + h] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    if (threadIdx.x == 0) {
        const uint64_t at = (uint64_t)a.beg + row - 1u;  // pos - 1
        uint8_t b = at < a.ref_len ? a.ref[at] : (uint8_t)'N';
        if (b >= 'a' && b <= 'z') b = (uint8_t)(b - 32);
        a.o_ref[k] = b == 'A' ? BV_BASE_A : b == 'C' ? BV_BASE_C : b == 'G' ? BV_BASE_G : b == 'T' ? BV_BASE_T : BV_BASE_OTHER;
    }
}

}  // namespace

// Per-engine state of bv_engine_pileup: the reference, the window's planes, and the completed pileup's host side.
struct BvPileupState {
    int device = 0;
    uint8_t *d_ref = nullptr, *d_records = nullptr, *d_meta = nullptr, *d_planes = nullptr, *d_depth = nullptr, *d_tok = nullptr, *d_text = nullptr,
            *d_slab = nullptr, *d_out = nullptr;
    uint8_t *d_inflated = nullptr;  // bv_engine_pileup_bgzf: the members' text, back to back (the sum of their ISIZE fields; kept, only grows)
    size_t inflated_cap = 0;
    size_t ref_cap = 0, rec_cap = 0, meta_cap = 0, planes_cap = 0, depth_cap = 0, tok_cap = 0, text_cap = 0, slab_cap = 0, out_cap = 0;
    bv_slab slab{};          // what the last bv_engine_pileup_rows filled
    bool have_slab = false;
    uint64_t ref_len = 0;
    bool have_ref = false;
    ChunkStage stage;
    // the completed pileup
    bool done = false;
    uint32_t rows = 0, n_samples = 0, beg = 0, max_rank = 0;
    uint64_t pitch = 0, text_bytes = 0;
    std::vector<uint32_t> depth, cov_rows;
    std::vector<BvPileupToken> tokens;  // sorted by (pos, sample)
};

void bv_pileup_state_free(BvPileupState *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    chunk_stage_free(t->stage);
    for (uint8_t *b : {t->d_ref, t->d_records, t->d_meta, t->d_planes, t->d_depth, t->d_tok, t->d_text, t->d_slab, t->d_out, t->d_inflated})
        if (b) (void)hipFree(b);
    delete t;
}

hipError_t bv_pileup_depth_launch(const uint16_t *rank, uint64_t pitch, uint32_t rows, uint32_t *depth, uint32_t *max_rank, hipStream_t st) {
    hipLaunchKernelGGL(bv_pileup_depth_kernel, dim3((rows + 3u) / 4u), dim3(256), 0, st, rank, pitch, rows, depth, max_rank);
    return hipGetLastError();
}

namespace {

struct PlaneOffsets {
    size_t cells, o_qual, o_mapq, o_rank, bytes;
    explicit PlaneOffsets(size_t c) : cells(c), o_qual(up256(c)), o_mapq(2 * up256(c)), o_rank(3 * up256(c)), bytes(3 * up256(c) + up256(2 * c)) {}
};

// host records to d_records through the pinned chunks, chunk k under the copy of chunk k + 1
int upload_records(bv_engine *e, BvPileupState *t, const uint8_t *src, uint64_t total, hipStream_t st) {
    int rc = chunk_stage_begin(e, t->stage, st);
    if (rc != BV_OK || total == 0) return rc;
    const size_t chunk = std::min<uint64_t>(total, chunk_limit_from_env("BASEVAR_AMD_PILEUP_CHUNK", (size_t)16 << 20));
    rc = chunk_stage_reserve(e, t->stage, chunk);
    if (rc != BV_OK) return rc;
    unsigned k = 0;
    for (uint64_t off = 0; off < total; off += chunk, ++k) {
        const unsigned s = k & 1u;
        const size_t len = (size_t)std::min<uint64_t>(chunk, total - off);
        if ((rc = chunk_stage_fill(e, t->stage, s)) != BV_OK) return rc;
        std::memcpy(t->stage.slot[s].h, src + off, len);
        if ((rc = chunk_stage_upload(e, t->stage, s, len, st)) != BV_OK) return rc;
        BV_HIP(e, hipMemcpyAsync(t->d_records + off, t->stage.slot[s].d, len, hipMemcpyDeviceToDevice, st));
        if ((rc = chunk_stage_done(e, t->stage, s, st)) != BV_OK) return rc;
    }
    return BV_OK;
}

// What one call piles up: run r is the bytes [run_at[2 r], run_at[2 r + 1]) behind `records` (device memory, complete on the stream)
struct PileJob {
    const char *who;             // "bv_engine_pileup: "
    const uint8_t *records;
    const uint64_t *run_at;      // host [n_runs][2]
    const uint32_t *run_sample;  // host [n_runs]
    uint64_t pitch;
    uint32_t n_runs, n_samples, beg, end;
};

int pileup(bv_engine *e, BvPileupState *t, const PileJob *in, const BvPileupQuery &q, uint32_t *n_covered, hipStream_t st) {
    const std::string who = in->who;
    const uint32_t n = in->n_samples, n_runs = in->n_runs, rows = in->end - in->beg + 1u;
    const PlaneOffsets P((size_t)rows * in->pitch);
    BV_HIP(e, hipSetDevice(t->device));
    // run_at u64 [n_runs][2], samp_run u32 [n + 1], per [n], tok_base u64 [n], text_base u64 [n]
    const size_t o_samp = up16(16ull * n_runs), o_per = o_samp + up16(4ull * (n + 1)), o_tokb = o_per + 32ull * n, o_textb = o_tokb + 8ull * n,
                 meta = o_textb + 8ull * n;
    int rc = grow_device(e, &t->d_meta, &t->meta_cap, meta);
    if (rc == BV_OK) rc = grow_device(e, &t->d_planes, &t->planes_cap, P.bytes);
    if (rc == BV_OK) rc = grow_device(e, &t->d_depth, &t->depth_cap, 8ull * rows);
    if (rc != BV_OK) return rc;
    std::vector<uint8_t> h(o_per, 0);
    uint32_t *h_samp = reinterpret_cast<uint32_t *>(h.data() + o_samp);
    if (n_runs) std::memcpy(h.data(), in->run_at, 16ull * n_runs);
    for (uint32_t r = 0; r < n_runs; ++r) h_samp[in->run_sample[r] + 1] = r + 1;
    for (uint32_t s = 0; s < n; ++s) h_samp[s + 1] = std::max(h_samp[s + 1], h_samp[s]);
    PileupArgs a;
    a.q = q;
    a.records = in->records;
    BV_HIP(e, hipMemcpyAsync(t->d_meta, h.data(), o_per, hipMemcpyHostToDevice, st));
    BV_HIP(e, hipMemsetAsync(t->d_planes, BV_CELL_N, P.o_qual, st));
    BV_HIP(e, hipMemsetAsync(t->d_planes + P.o_qual, 0, P.bytes - P.o_qual, st));
    a.run_at = reinterpret_cast<const uint64_t *>(t->d_meta); a.samp_run = reinterpret_cast<const uint32_t *>(t->d_meta + o_samp);
    a.ref = t->d_ref;
    a.planes = t->d_planes; a.plane_bytes = P.o_qual; a.pitch = in->pitch;
    a.per = reinterpret_cast<BvPileupSample *>(t->d_meta + o_per);
    a.tok_base = reinterpret_cast<const uint64_t *>(t->d_meta + o_tokb); a.text_base = reinterpret_cast<const uint64_t *>(t->d_meta + o_textb);
    a.tokens = nullptr; a.text = nullptr;
    a.rows = rows;
    const size_t lds = 4ull * ((rows + 31u) / 32u);
    hipLaunchKernelGGL(bv_pileup_kernel<false>, dim3(n), dim3(64), lds, st, a);
    BV_HIP(e, hipGetLastError());
    uint32_t *d_depth = reinterpret_cast<uint32_t *>(t->d_depth);
    hipLaunchKernelGGL(bv_pileup_depth_kernel, dim3((rows + 3u) / 4u), dim3(256), 0, st, reinterpret_cast<const uint16_t *>(t->d_planes + P.o_rank), a.pitch, rows, d_depth, d_depth + rows);
    BV_HIP(e, hipGetLastError());
    std::vector<BvPileupSample> per(n);
    std::vector<uint32_t> dm(2ull * rows);
    BV_HIP(e, hipMemcpyAsync(per.data(), a.per, 32ull * n, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipMemcpyAsync(dm.data(), d_depth, 8ull * rows, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    for (uint32_t s = 0; s < n; ++s) {
        if (per[s].status == BV_PILEUP_OK) continue;
        const std::string where = "sample " + std::to_string(s) + ", run " + std::to_string(per[s].run) + ", the record at byte " + std::to_string(per[s].at) + " of the run";
        if (per[s].status == BV_PILEUP_BAD_BASE) return fail(e, BV_ERR_SITE, std::string(bv_pileup_status_text(BV_PILEUP_BAD_BASE)) + " (" + who + where + ")");
        return fail(e, BV_ERR_DATA, who + where + ": " + bv_pileup_status_text(per[s].status));
    }
    // the tokens' places: a running sum in sample order
    std::vector<uint64_t> base(2ull * n);
    uint64_t n_tok = 0, text_bytes = 0;
    for (uint32_t s = 0; s < n; ++s) {
        base[s] = n_tok; base[n + s] = text_bytes;
        n_tok += per[s].n_tokens; text_bytes += per[s].text_bytes;
    }
    t->tokens.assign(n_tok, BvPileupToken());
    if (n_tok) {
        rc = grow_device(e, &t->d_tok, &t->tok_cap, sizeof(BvPileupToken) * n_tok);
        if (rc == BV_OK) rc = grow_device(e, &t->d_text, &t->text_cap, up256(text_bytes));
        if (rc != BV_OK) return rc;
        BV_HIP(e, hipMemcpyAsync(t->d_meta + o_tokb, base.data(), 16ull * n, hipMemcpyHostToDevice, st));
        a.tokens = reinterpret_cast<BvPileupToken *>(t->d_tok); a.text = t->d_text;
        hipLaunchKernelGGL(bv_pileup_kernel<true>, dim3(n), dim3(64), lds, st, a);
        BV_HIP(e, hipGetLastError());
        BV_HIP(e, hipMemcpyAsync(t->tokens.data(), t->d_tok, sizeof(BvPileupToken) * n_tok, hipMemcpyDeviceToHost, st));
        BV_HIP(e, hipStreamSynchronize(st));
        std::stable_sort(t->tokens.begin(), t->tokens.end(), [](const BvPileupToken &x, const BvPileupToken &y) {
            return x.pos != y.pos ? x.pos < y.pos : x.sample < y.sample;
        });
    }
    t->rows = rows; t->n_samples = n; t->beg = in->beg; t->pitch = in->pitch; t->text_bytes = text_bytes;
    t->depth.assign(dm.begin(), dm.begin() + rows);
    t->cov_rows.clear();
    t->max_rank = 0;
    for (uint32_t r = 0; r < rows; ++r) {
        if (dm[r]) t->cov_rows.push_back(r);
        t->max_rank = std::max(t->max_rank, dm[rows + r]);
    }
    *n_covered = (uint32_t)t->cov_rows.size();
    t->done = true;
    return BV_OK;
}

}  // namespace

// what bv_pileup_text.hip reads of the state: the reference, and the completed pileup where it lies
void bv_pileup_view(const BvPileupState *t, BvPileupView *v) {
    *v = BvPileupView();
    if (!t) return;
    v->have_ref = t->have_ref; v->d_ref = t->d_ref; v->ref_len = t->ref_len;
    if (!t->done) return;
    const PlaneOffsets P((size_t)t->rows * t->pitch);
    v->done = true;
    v->cell = t->d_planes; v->qual = t->d_planes + P.o_qual; v->mapq = t->d_planes + P.o_mapq;
    v->rank = reinterpret_cast<const uint16_t *>(t->d_planes + P.o_rank);
    v->pitch = t->pitch; v->rows = t->rows; v->n_samples = t->n_samples; v->beg = t->beg;
    v->depth = t->depth.data();
    v->tokens = t->tokens.data(); v->n_tokens = t->tokens.size();
    v->d_text = t->d_text; v->text_bytes = t->text_bytes;
}

extern "C" {

uint32_t bv_pileup_max_rows(void) { return BV_PILEUP_MAX_ROWS; }

int bv_engine_pileup_set_reference(bv_engine *e, const char *seq, uint64_t len) {
    const std::string who = "bv_engine_pileup_set_reference: ";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    if (!seq && len) return fail(e, BV_ERR_INVALID_ARG, who + "null seq");
    BvPileupState *t = engine_state(e, e->pileup);
    t->have_ref = false;
    t->done = t->have_slab = false;
    BV_HIP(e, hipSetDevice(t->device));
    BV_HIP(e, hipStreamSynchronize(e->stream));
    if (len) {
        const int rc = grow_device(e, &t->d_ref, &t->ref_cap, up256(len));
        if (rc != BV_OK) return rc;
        BV_HIP(e, hipMemcpy(t->d_ref, seq, len, hipMemcpyHostToDevice));
        t->have_ref = true;
    }
    t->ref_len = len;
    return BV_OK;
}

int bv_engine_pileup(bv_engine *e, const bv_pileup_reads *in, uint32_t *n_covered, void *stream_) {
    const std::string who = "bv_engine_pileup: ";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    if (e->pileup) e->pileup->done = e->pileup->have_slab = false;  // whatever comes of this call, the last pileup is gone
    if (!in || !n_covered) return fail(e, BV_ERR_INVALID_ARG, who + "null reads/n_covered");
    if (in->reserved_) return fail(e, BV_ERR_INVALID_ARG, who + "reserved_ must be zero");
    if (in->mem_kind != BV_MEM_HOST && in->mem_kind != BV_MEM_DEVICE) return fail(e, BV_ERR_INVALID_ARG, who + "mem_kind must be BV_MEM_HOST or BV_MEM_DEVICE");
    if (in->n_samples == 0 || in->pitch < in->n_samples || (in->pitch & 15ull)) return fail(e, BV_ERR_INVALID_ARG, who + "pitch must be >= n_samples >= 1 and a multiple of 16");
    if (in->tid < 0) return fail(e, BV_ERR_INVALID_ARG, who + "tid must not be negative");
    if (in->end >= in->beg && (uint64_t)in->end - in->beg + 1u > BV_PILEUP_MAX_ROWS)
        return fail(e, BV_ERR_TOO_LARGE, who + "a window of " + std::to_string((uint64_t)in->end - in->beg + 1u) + " rows: more than bv_pileup_max_rows() = " + std::to_string(BV_PILEUP_MAX_ROWS));
    uint32_t gb = 0, ge = 0;
    if (!bv_pileup_step(in->region_beg, in->region_end, in->beg, in->end, &gb, &ge))
        return fail(e, BV_ERR_INVALID_ARG, who + "a window must lie inside the region and must not cross the 500 kb step grid laid out from region_beg");
    if (in->n_runs) {
        if (!in->run_off || !in->run_sample) return fail(e, BV_ERR_INVALID_ARG, who + "null run_off/run_sample");
        for (uint32_t r = 0; r < in->n_runs; ++r) {
            if (in->run_off[r + 1] < in->run_off[r]) return fail(e, BV_ERR_INVALID_ARG, who + "run_off out of order at run " + std::to_string(r));
            if (in->run_sample[r] >= in->n_samples) return fail(e, BV_ERR_INVALID_ARG, who + "run_sample of run " + std::to_string(r) + " is beyond n_samples");
            if (r && in->run_sample[r] < in->run_sample[r - 1]) return fail(e, BV_ERR_INVALID_ARG, who + "run_sample descends at run " + std::to_string(r));
        }
        if (!in->records && in->run_off[in->n_runs] != in->run_off[0]) return fail(e, BV_ERR_INVALID_ARG, who + "null records");
    }
    BvPileupState *t = e->pileup;
    if (!t || !t->have_ref) return fail(e, BV_ERR_INVALID_ARG, who + "no reference set: bv_engine_pileup_set_reference comes first");
    if (in->end > t->ref_len) return fail(e, BV_ERR_INVALID_ARG, who + "the window ends beyond the reference's " + std::to_string(t->ref_len) + " bases");
    BvPileupQuery q;
    bv_pileup_query(in->tid, in->beg, in->end, gb, ge, in->mapq_thd, t->ref_len, &q);
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    // neighbours of one offset array as the pairs the kernels read
    std::vector<uint64_t> run_at(2ull * in->n_runs);
    for (uint32_t r = 0; r < in->n_runs; ++r) { run_at[2ull * r] = in->run_off[r]; run_at[2ull * r + 1] = in->run_off[r + 1]; }
    PileJob job{"bv_engine_pileup: ", in->records, run_at.data(), in->run_sample, in->pitch, in->n_runs, in->n_samples, in->beg, in->end};
    if (in->mem_kind == BV_MEM_HOST) {
        const uint64_t rec_lo = in->n_runs ? in->run_off[0] : 0, total = in->n_runs ? in->run_off[in->n_runs] - rec_lo : 0;
        BV_HIP(e, hipSetDevice(t->device));
        int rc = grow_device(e, &t->d_records, &t->rec_cap, up256(total + 16));
        if (rc == BV_OK) rc = upload_records(e, t, in->records + rec_lo, total, st);
        if (rc != BV_OK) return rc;
        job.records = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(t->d_records) - rec_lo);
    }
    return pileup(e, t, &job, q, n_covered, st);
}

int bv_engine_pileup_bgzf(bv_engine *e, const bv_pileup_bgzf *in, uint32_t *n_covered, void *stream_) {
    const std::string who = "bv_engine_pileup_bgzf: ";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    if (e->pileup) e->pileup->done = e->pileup->have_slab = false;  // whatever comes of this call, the last pileup is gone
    if (!in || !n_covered) return fail(e, BV_ERR_INVALID_ARG, who + "null members-and-runs/n_covered");
    if (in->reserved_ || in->members.reserved_) return fail(e, BV_ERR_INVALID_ARG, who + "reserved_ must be zero");
    if (in->n_samples == 0 || in->pitch < in->n_samples || (in->pitch & 15ull)) return fail(e, BV_ERR_INVALID_ARG, who + "pitch must be >= n_samples >= 1 and a multiple of 16");
    if (in->tid < 0) return fail(e, BV_ERR_INVALID_ARG, who + "tid must not be negative");
    if (in->end >= in->beg && (uint64_t)in->end - in->beg + 1u > BV_PILEUP_MAX_ROWS)
        return fail(e, BV_ERR_TOO_LARGE, who + "a window of " + std::to_string((uint64_t)in->end - in->beg + 1u) + " rows: more than bv_pileup_max_rows() = " + std::to_string(BV_PILEUP_MAX_ROWS));
    uint32_t gb = 0, ge = 0;
    if (!bv_pileup_step(in->region_beg, in->region_end, in->beg, in->end, &gb, &ge))
        return fail(e, BV_ERR_INVALID_ARG, who + "a window must lie inside the region and must not cross the 500 kb step grid laid out from region_beg");
    const bv_bgzf_members *mb = &in->members;
    const uint32_t n_mem = mb->n_members, n_runs = in->n_runs;
    if (n_mem && (!mb->data || !mb->member_off)) return fail(e, BV_ERR_INVALID_ARG, who + "null data/member_off");
    if (n_runs && !in->runs) return fail(e, BV_ERR_INVALID_ARG, who + "null runs");
    std::vector<BvBgzfMember> hd;
    std::vector<uint8_t> pre;
    int rc = bv_bgzf_headers(e, "bv_engine_pileup_bgzf", mb, hd, pre);
    if (rc != BV_OK) return rc;
    std::vector<uint64_t> dst_off(n_mem + 1ull, 0);
    for (uint32_t k = 0; k < n_mem; ++k) dst_off[k + 1] = dst_off[k] + hd[k].isize;
    std::vector<uint64_t> run_at(2ull * n_runs);
    std::vector<uint32_t> run_sample(n_runs);
    for (uint32_t r = 0; r < n_runs; ++r) {
        const bv_pileup_bgzf_run &u = in->runs[r];
        const std::string run = "run " + std::to_string(r);
        if (u.reserved_) return fail(e, BV_ERR_INVALID_ARG, who + run + ": reserved_ must be zero");
        if (u.sample >= in->n_samples) return fail(e, BV_ERR_INVALID_ARG, who + "sample of " + run + " is beyond n_samples");
        if (r && u.sample < in->runs[r - 1].sample) return fail(e, BV_ERR_INVALID_ARG, who + "sample descends at " + run);
        if (u.n_members == 0) return fail(e, BV_ERR_INVALID_ARG, who + run + " has no member");
        if ((uint64_t)u.first_member + u.n_members > n_mem)
            return fail(e, BV_ERR_INVALID_ARG, who + run + ": members " + std::to_string(u.first_member) + " + " + std::to_string(u.n_members) + " are beyond the " + std::to_string(n_mem) + " given");
        // (a member that its header already refuses has no ISIZE to hold a cut point to: it ends the call as BV_ERR_DATA below)
        const uint32_t last = u.first_member + u.n_members - 1u;
        if (pre[u.first_member] == BV_BGZF_OK && u.begin > hd[u.first_member].isize)
            return fail(e, BV_ERR_INVALID_ARG, who + run + ": begin " + std::to_string(u.begin) + " is above its first member's ISIZE " + std::to_string(hd[u.first_member].isize));
        if (pre[last] == BV_BGZF_OK && u.end > hd[last].isize)
            return fail(e, BV_ERR_INVALID_ARG, who + run + ": end " + std::to_string(u.end) + " is above its last member's ISIZE " + std::to_string(hd[last].isize));
        if (u.n_members == 1 && u.begin > u.end) return fail(e, BV_ERR_INVALID_ARG, who + run + ": begin " + std::to_string(u.begin) + " > end " + std::to_string(u.end) + " inside one member");
        run_at[2ull * r] = dst_off[u.first_member] + u.begin;
        run_at[2ull * r + 1] = std::max(run_at[2ull * r], dst_off[last] + u.end);  // (behind a refused member only: the call ends before the pile)
        run_sample[r] = u.sample;
    }
    BvPileupState *t = e->pileup;
    if (!t || !t->have_ref) return fail(e, BV_ERR_INVALID_ARG, who + "no reference set: bv_engine_pileup_set_reference comes first");
    if (in->end > t->ref_len) return fail(e, BV_ERR_INVALID_ARG, who + "the window ends beyond the reference's " + std::to_string(t->ref_len) + " bases");
    BvPileupQuery q;
    bv_pileup_query(in->tid, in->beg, in->end, gb, ge, in->mapq_thd, t->ref_len, &q);
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    BV_HIP(e, hipSetDevice(t->device));
    if (n_mem) {
        // the members once each, back to back; the call returns with their statuses on the host: the one wait before the pile
        if ((rc = grow_device(e, &t->d_inflated, &t->inflated_cap, up256(dst_off[n_mem] + 16))) != BV_OK) return rc;
        std::vector<uint8_t> status(n_mem);
        if ((rc = bv_bgzf_inflate_placed(e, mb, hd, pre, dst_off.data(), t->d_inflated, status.data(), st)) != BV_OK) return rc;
        for (uint32_t k = 0; k < n_mem; ++k) {
            if (status[k] == BV_BGZF_OK) continue;
            static const char *const kWhat[] = {"ok", "bad header", "bad DEFLATE stream", "bad size", "bad CRC"};
            std::string used = "used by no run";
            for (uint32_t r = 0; r < n_runs; ++r)
                if (k >= in->runs[r].first_member && k - in->runs[r].first_member < in->runs[r].n_members) {
                    used = "first used by sample " + std::to_string(in->runs[r].sample) + ", run " + std::to_string(r);
                    break;
                }
            return fail(e, BV_ERR_DATA, who + "member " + std::to_string(k) + " did not inflate: status " + std::to_string(status[k]) + " (" +
                                            (status[k] < 5 ? kWhat[status[k]] : "?") + "), " + used);
        }
    }
    const PileJob job{"bv_engine_pileup_bgzf: ", t->d_inflated, run_at.data(), run_sample.data(), in->pitch, n_runs, in->n_samples, in->beg, in->end};
    return pileup(e, t, &job, q, n_covered, st);
}

int bv_engine_pileup_fetch(bv_engine *e, bv_pileup_result *out, void *stream_) {
    const std::string who = "bv_engine_pileup_fetch: ";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    if (!out) return fail(e, BV_ERR_INVALID_ARG, who + "null result");
    BvPileupState *t = e->pileup;
    if (!t || !t->done) return fail(e, BV_ERR_INVALID_ARG, who + "no completed bv_engine_pileup before it");
    const PlaneOffsets P((size_t)t->rows * t->pitch);
    out->cells = P.cells; out->rows = t->rows; out->n_tokens = t->tokens.size(); out->text_bytes = t->text_bytes;
    if (out->reserved_) return fail(e, BV_ERR_INVALID_ARG, who + "reserved_ must be zero");
    if (out->mem_kind != BV_MEM_HOST && out->mem_kind != BV_MEM_DEVICE) return fail(e, BV_ERR_INVALID_ARG, who + "mem_kind must be BV_MEM_HOST or BV_MEM_DEVICE");
    if (((out->cell || out->qual || out->mapq || out->rank) && out->cells_capacity < out->cells) || (out->depth && out->rows_capacity < out->rows) ||
        (out->tokens && out->tokens_capacity < out->n_tokens) || (out->text && out->text_capacity < out->text_bytes))
        return fail(e, BV_ERR_INVALID_ARG, who + "a capacity is below what the pileup holds: " + std::to_string(out->cells) + " cells, " + std::to_string(out->rows) +
                                               " rows, " + std::to_string(out->n_tokens) + " tokens, " + std::to_string(out->text_bytes) + " bytes of text");
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    BV_HIP(e, hipSetDevice(t->device));
    const bool host = out->mem_kind == BV_MEM_HOST;
    const hipMemcpyKind from_dev = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, from_host = host ? hipMemcpyHostToHost : hipMemcpyHostToDevice;
    if (out->cell) BV_HIP(e, hipMemcpyAsync(out->cell, t->d_planes, P.cells, from_dev, st));
    if (out->qual) BV_HIP(e, hipMemcpyAsync(out->qual, t->d_planes + P.o_qual, P.cells, from_dev, st));
    if (out->mapq) BV_HIP(e, hipMemcpyAsync(out->mapq, t->d_planes + P.o_mapq, P.cells, from_dev, st));
    if (out->rank) BV_HIP(e, hipMemcpyAsync(out->rank, t->d_planes + P.o_rank, 2 * P.cells, from_dev, st));
    if (out->depth) BV_HIP(e, hipMemcpyAsync(out->depth, t->depth.data(), 4ull * t->rows, from_host, st));
    if (out->tokens && !t->tokens.empty()) BV_HIP(e, hipMemcpyAsync(out->tokens, t->tokens.data(), sizeof(BvPileupToken) * t->tokens.size(), from_host, st));
    if (out->text && t->text_bytes) BV_HIP(e, hipMemcpyAsync(out->text, t->d_text, t->text_bytes, from_dev, st));
    BV_HIP(e, hipStreamSynchronize(st));
    return BV_OK;
}

int bv_engine_pileup_rows(bv_engine *e, int tagged, bv_slab *slab, uint32_t *pos, uint32_t *depth) {
    const std::string who = "bv_engine_pileup_rows: ";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    if (!slab) return fail(e, BV_ERR_INVALID_ARG, who + "null slab");
    BvPileupState *t = e->pileup;
    if (!t || !t->done) return fail(e, BV_ERR_INVALID_ARG, who + "no completed bv_engine_pileup before it");
    if (tagged && t->max_rank > BV_RPR_TAG_MAX_RANK)
        return fail(e, BV_ERR_INVALID_ARG, who + "a read-position rank of " + std::to_string(t->max_rank) + " does not fit the tagged layout (BV_RPR_TAG_MAX_RANK)");
    const uint32_t n = (uint32_t)t->cov_rows.size();
    std::memset(slab, 0, sizeof *slab);
    slab->n_sites = n; slab->n_samples = t->n_samples; slab->pitch = t->pitch; slab->mem_kind = BV_MEM_DEVICE; slab->layout = tagged ? BV_SLAB_RPR_TAGGED : 0u;
    for (uint32_t k = 0; k < n; ++k) {
        if (pos) pos[k] = t->beg + t->cov_rows[k];
        if (depth) depth[k] = t->depth[t->cov_rows[k]];
    }
    t->slab = *slab;
    t->have_slab = true;
    if (n == 0) return BV_OK;
    t->have_slab = false;
    const PlaneOffsets W((size_t)t->rows * t->pitch), S((size_t)n * t->pitch);
    const size_t o_ref = S.bytes, o_row = o_ref + up256(n);
    BV_HIP(e, hipSetDevice(t->device));
    const int rc = grow_device(e, &t->d_slab, &t->slab_cap, o_row + 4ull * n);
    if (rc != BV_OK) return rc;
    hipStream_t st = e->stream;
    BV_HIP(e, hipMemcpyAsync(t->d_slab + o_row, t->cov_rows.data(), 4ull * n, hipMemcpyHostToDevice, st));
    GatherArgs g;
    g.cell = t->d_planes; g.qual = t->d_planes + W.o_qual; g.mapq = t->d_planes + W.o_mapq; g.rank = reinterpret_cast<const uint16_t *>(t->d_planes + W.o_rank);
    g.o_cell = t->d_slab; g.o_qual = t->d_slab + S.o_qual; g.o_mapq = t->d_slab + S.o_mapq; g.o_rank = reinterpret_cast<uint16_t *>(t->d_slab + S.o_rank);
    g.o_ref = t->d_slab + o_ref;
    g.row_of = reinterpret_cast<const uint32_t *>(t->d_slab + o_row);
    g.ref = t->d_ref; g.ref_len = t->ref_len; g.pitch = t->pitch; g.beg = t->beg; g.tagged = tagged ? 1u : 0u;
    hipLaunchKernelGGL(bv_pileup_gather_kernel, dim3(n), dim3(256), 0, st, g);
    BV_HIP(e, hipGetLastError());
    BV_HIP(e, hipStreamSynchronize(st));
    slab->base_strand = g.o_cell; slab->qual = g.o_qual; slab->mapq = g.o_mapq; slab->rpr = g.o_rank; slab->ref_base = g.o_ref;
    t->slab = *slab;
    t->have_slab = true;
    return BV_OK;
}

int bv_engine_pileup_submit(bv_engine *e, uint32_t first, uint32_t n, const uint8_t *group_id, uint32_t n_groups, bv_site_result *out,
                            bv_group_result *gout, uint8_t *cell, uint8_t *phred, void *stream_) {
    const std::string who = "bv_engine_pileup_submit: ";
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    BvPileupState *t = e->pileup;
    if (!t || !t->done || !t->have_slab) return fail(e, BV_ERR_INVALID_ARG, who + "no bv_engine_pileup_rows since the last pileup");
    if (n == 0 || !out || (n_groups && (!gout || !group_id))) return fail(e, BV_ERR_INVALID_ARG, who + "n == 0 or null out/gout/group_id");
    if ((uint64_t)first + n > t->slab.n_sites)
        return fail(e, BV_ERR_INVALID_ARG, who + "rows " + std::to_string(first) + " + " + std::to_string(n) + " are beyond the slab's " + std::to_string(t->slab.n_sites));
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    BV_HIP(e, hipSetDevice(t->device));
    const uint32_t N = t->slab.n_samples;
    const size_t o_gout = up256(sizeof(bv_site_result) * n), o_gid = o_gout + up256(sizeof(bv_group_result) * n * n_groups);
    int rc = grow_device(e, &t->d_out, &t->out_cap, o_gid + up256(N));
    if (rc != BV_OK) return rc;
    if (n_groups) BV_HIP(e, hipMemcpyAsync(t->d_out + o_gid, group_id, N, hipMemcpyHostToDevice, st));
    bv_slab s = t->slab;
    const size_t at = (size_t)first * s.pitch;
    s.n_sites = n;
    s.base_strand += at; s.qual += at; s.mapq += at; s.rpr += at; s.ref_base += first;
    s.group_id = n_groups ? t->d_out + o_gid : nullptr; s.n_groups = n_groups;
    bv_site_result *d_out = reinterpret_cast<bv_site_result *>(t->d_out);
    bv_group_result *d_gout = n_groups ? reinterpret_cast<bv_group_result *>(t->d_out + o_gout) : nullptr;
    rc = bv_engine_submit(e, &s, d_out, d_gout, st);
    if (rc != BV_OK) return rc;
    rc = bv_engine_join(e, st);
    if (rc != BV_OK) return rc;
    BV_HIP(e, hipMemcpyAsync(out, d_out, sizeof(bv_site_result) * n, hipMemcpyDeviceToHost, st));
    if (n_groups) BV_HIP(e, hipMemcpyAsync(gout, d_gout, sizeof(bv_group_result) * n * n_groups, hipMemcpyDeviceToHost, st));
    if (cell) BV_HIP(e, hipMemcpy2DAsync(cell, N, s.base_strand, s.pitch, N, n, hipMemcpyDeviceToHost, st));
    if (phred) BV_HIP(e, hipMemcpy2DAsync(phred, N, s.qual, s.pitch, N, n, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    return BV_OK;
}

}  // extern "C"
