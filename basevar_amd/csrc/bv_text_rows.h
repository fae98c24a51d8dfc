// bv_text_rows.h -- what the two parsers of batchfile text rows share: bv_engine_text_parse and its kin (bv_text.hip), which take
// one row of every file per position at once, and the parse job (bv_text_job.hip, include/basevar_amd_text_job.h), which takes
// the files a few at a time.  The arguments and helpers of the walk of one row by one wave
// (bv_text_row_walk_body.h), the arrays of a parse (ParseBufs), the per-engine
// state (BvTextState) and the host steps around the kernels.  Included by those two files only.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/basevar_amd.h"
#include "bv_chunk_stage.h"

namespace {

constexpr uint32_t kPrefixFail = 1u;  // d_pstate bits: the field count or the first four fields are not the strict form
constexpr uint32_t kTokenFail = 2u;   //                a per-sample token is not the strict form
constexpr uint32_t kMaxPrefix = 512;  // bytes of CHROM \t POS \t REF \t Depth \t the device looks at; longer -> host
constexpr size_t kChunkBytes = (size_t)128 << 20;  // text bytes per staged chunk (two chunks in flight)

struct TextParseArgs {
    const char *text;          // the chunk: byte k is text byte chunk_base + k
    const uint64_t *row_beg;   // [n_rows] absolute offset of every row's first byte (device) ...
    const uint64_t *row_end;   // [n_rows] ... and of the byte behind its '\n' (bv_engine_text_parse: row_beg + 1, rows are contiguous)
    const uint32_t *foff;      // [n_files] sample offset of file f inside the row
    const uint32_t *fsamp;     // [n_files]
    uint64_t chunk_base;
    uint32_t row_first, n_rows_chunk, n_files;
    uint64_t pitch;
    uint8_t *bs, *q, *mq, *st, *ref, *rowflag;
    uint16_t *rp;
    uint32_t *depth, *pstate, *pmax;
};

__device__ __forceinline__ bool is_digit(char c) { return c >= '0' && c <= '9'; }
__device__ __forceinline__ bool is_sep(char c) { return c == ' ' || c == '\t' || c == '\n'; }

// digits [p, first separator): 1..max_digits of them, value <= max_value -> value, else -1
__device__ __forceinline__ int parse_uint_token(const char *p, int max_digits, int max_value) {
    int v = 0, n = 0;
    for (;; ++n) {
        const char c = p[n];
        if (is_sep(c)) break;
        if (!is_digit(c) || n == max_digits) return -1;
        v = v * 10 + (c - '0');
    }
    return (n == 0 || v > max_value) ? -1 : v;
}

__device__ __forceinline__ uint8_t base_code_dev(char c) {
    switch (c) {
        case 'A': case 'a': return BV_BASE_A;
        case 'C': case 'c': return BV_BASE_C;
        case 'G': case 'g': return BV_BASE_G;
        case 'T': case 't': return BV_BASE_T;
        default: return BV_BASE_OTHER;
    }
}

}  // namespace

// The device arrays of one parse of P positions x F files.
struct ParseBufs {
    uint8_t *bs, *q, *mq, *stp, *ref, *rowflag;
    uint16_t *rp;
    uint32_t *depth, *pstate, *pmax, *foff, *fsamp;
    uint64_t *d_off;  // [2 * (P * F + 1)]: row_off [P * F + 1] of bv_engine_text_parse; row begins [P * F], then row ends, of _parse_bgzf
    uint64_t pitch;
};

// The parse job that is open on the engine (bv_text_job.hip): what bv_engine_text_job_begin fixed, the files added so far, and
// the positions' heads.  `open` falls with every parse_begin and bgzf_runs_begin: a parse replaces the one before it.
struct BvTextJob {
    bool open = false;
    bool tokens = false;                    // the token mode at begin: it holds for the whole job
    uint32_t P = 0, F = 0, n_samples = 0, n_groups = 0, n_added = 0;
    std::vector<uint32_t> file_samples;
    std::vector<uint8_t> added;             // [F]
    std::vector<uint8_t> group_id;
    bool has_gid = false;
    ParseBufs pb;
};

// Per-engine state of the text path: the parsed planes of the last bv_engine_text_parse, the slab handed to the calling kernels,
// the staging of the text chunks (bv_chunk_stage.h) and what the host learnt from the parse.
struct BvTextState {
    int device = 0;
    bv_impl::ChunkStage chunks;
    uint8_t *d_planes = nullptr;            // parsed rows: bs, q, mq, st [cap][pitch], rp [cap][pitch] u16, ref [cap]
    size_t planes_bytes = 0;
    uint8_t *d_sub = nullptr;               // the submitted slab: bs, q, mq [cap][pitch], rp [cap][pitch] u16, ref [cap]
    size_t sub_bytes = 0;
    uint32_t sub_rows = 0, sub_samples = 0; // rows of the last submit that stand in d_sub (bv_text_kept_rows); 0: none
    uint64_t sub_pitch = 0;
    uint32_t sub_layout = 0;                // bv_slab.layout of the last submit's slab (bv_engine_text_last_layout)
    uint8_t *d_aux = nullptr;               // depth, pstate, pmax [n_pos] u32, rowflag [n_rows], row_off [n_rows + 1], foff/fsamp
    size_t aux_bytes = 0;
    uint8_t *d_misc = nullptr;              // submit: src [n] i32, host rows, records
    size_t misc_bytes = 0;
    uint8_t *d_gid = nullptr;
    size_t gid_bytes = 0;
    // the pending parse
    bool parsed = false;
    uint32_t n_pos = 0, n_files = 0, n_samples = 0, n_groups = 0;
    uint64_t pitch = 0;
    std::vector<uint8_t> pos_state;         // BV_TEXT_SKIP / BV_TEXT_HOST / 0 per position
    std::vector<uint32_t> pos_max_rank;
    std::vector<uint8_t> group_id;
    bool has_gid = false;
    std::vector<uint32_t> h_foff;           // sample offset of every file (what parse_begin uploads)
    // bv_engine_text_parse_bgzf: the inflated runs, the line index, and what bv_engine_text_rows_fetch gathers
    bool bgzf_rows = false;                 // the last parse was a _parse_bgzf: d_btext and the row begins / ends stand
    const uint64_t *bz_row_beg = nullptr, *bz_row_end = nullptr;  // ... where they stand (inside d_aux) ...
    const uint8_t *bz_rowflag = nullptr;    // ... and the rows' BV_TEXT_INDEL flags
    uint8_t *d_btext = nullptr;             // file f's run inflated back to back, one spare byte behind each run
    size_t btext_bytes = 0;
    uint8_t *d_lines = nullptr;             // LineFile [n_files], newline counts / prefixes per tile, n_pos
    size_t lines_bytes = 0;
    uint8_t *d_fetch = nullptr;             // rows_fetch: pos_state [n_pos], len u32 [n_rows], off u64 [n_rows + 1], the bytes
    size_t fetch_bytes = 0;
    uint8_t *d_rrows = nullptr;             // _parse_bgzf_region: row begins, then row ends, of (n_pos + 1) * n_files rows
    size_t rrows_bytes = 0;
    // the parse job (include/basevar_amd_text_job.h)
    BvTextJob job;
    uint8_t *d_heads = nullptr;             // heads [P][kMaxPrefix], then their lengths u32 [P] (0: not captured yet)
    size_t heads_bytes = 0;
};

namespace bv_impl {
// bv_text.hip, for the job as for the parses of that file.
// Sized, cleared (a parsed row is all 'N' where the text leaves nothing) and with the files' sample offsets in place.
int text_parse_begin(bv_engine *e, BvTextState *t, uint32_t P, uint32_t F, const uint32_t *file_samples, uint32_t n_samples, hipStream_t st,
                     ParseBufs *b);
// The strands into the cells, then what the host needs to know of every position.
int text_parse_finish(bv_engine *e, BvTextState *t, uint32_t P, uint32_t F, uint32_t n_samples, const uint8_t *group_id, uint32_t n_groups,
                      uint8_t *row_state, hipStream_t st, const ParseBufs &b);
// What every parse entry point asks of file_samples and group_id / n_groups; *n_samples = the samples of all files.
int text_check_samples_groups(bv_engine *e, const char *who, const uint32_t *file_samples, uint32_t F, const uint8_t *group_id, uint32_t n_groups,
                              uint64_t *n_samples);
// What every call that takes a bv_text_rows asks of it: the pointers, reserved_ and the counts; and the rows in order, inside the
// text, each ending in '\n'
int text_check_rows_head(bv_engine *e, const char *who, const bv_text_rows *rows);
int text_check_rows_off(bv_engine *e, const char *who, const bv_text_rows *rows);
BvTextState *text_state(bv_engine *e);  // e->text, created if it is missing
}  // namespace bv_impl
