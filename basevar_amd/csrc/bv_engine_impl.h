// bv_engine_impl.h -- the engine as its own translation units see it (bv_engine.hip, bv_engine_rows.hip, bv_engine_tiles.hip,
// bv_text.hip, bv_inflate.hip, bv_deflate.hip, bv_vcf.hip, bv_pileup.hip, bv_pileup_text.hip, bv_record_text.hip, bv_indel_tally.hip): struct bv_engine, the error path, and the plumbing every entry point shares.  (bv_vcf.hip and
// bv_pileup_text.hip share two more headers: bv_device_text.h, the text they leave on the device, and bv_text_image.h, the
// kernels' side of writing it.)  Host-only; the
// files that hold the calling kernels (pass 1, pass 2, tiles) know the launch-argument blocks of bv_kernels.h and nothing of this.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "bv_kernels.h"

struct BvTextState;   // bv_engine_text_parse / _submit (bv_text.hip)
void bv_text_state_free(BvTextState *t);
struct BvBgzfState;   // bv_engine_bgzf_inflate (bv_inflate.hip)
void bv_bgzf_state_free(BvBgzfState *t);
struct BvDeflateState;  // bv_engine_bgzf_deflate (bv_deflate.hip)
void bv_deflate_state_free(BvDeflateState *t);
struct BvVcfState;      // bv_engine_vcf_format (bv_vcf.hip)
void bv_vcf_state_free(BvVcfState *t);
struct BvPileupState;   // bv_engine_pileup (bv_pileup.hip)
void bv_pileup_state_free(BvPileupState *t);
struct BvPtextState;    // bv_engine_pileup_text (bv_pileup_text.hip)
void bv_ptext_state_free(BvPtextState *t);
struct BvRtextState;    // bv_engine_cvg_format / bv_engine_vcf_format_records (bv_record_text.hip)
void bv_rtext_state_free(BvRtextState *t);
struct BvIndelState;    // bv_engine_indel_tally (bv_indel_tally.hip)
void bv_indel_state_free(BvIndelState *t);
// The last completed bv_engine_indel_tally, as it lies (bv_indel_tally.hip): bv_engine_cvg_format_tallied reads it
struct BvIndelView {
    bool done = false;
    uint32_t n = 0;
    const uint8_t *d_text = nullptr;   // device: the columns back to back
    const uint64_t *d_off = nullptr;   // device [n + 1]
    const uint8_t *flag = nullptr;     // host [n]
};
void bv_indel_view(const BvIndelState *t, BvIndelView *v);
struct BvTextTokState;  // bv_engine_text_tokens (bv_text_tokens.hip)
void bv_text_tok_state_free(BvTextTokState *t);
struct BvPileupToken;   // bv_pileup_core.h
// The last completed bv_engine_pileup and the uploaded reference, as they lie (bv_pileup.hip): have_ref / done say what is there
struct BvPileupView {
    bool have_ref = false, done = false;
    const uint8_t *d_ref = nullptr;
    uint64_t ref_len = 0;
    const uint8_t *cell = nullptr, *qual = nullptr, *mapq = nullptr;  // device [rows][pitch]
    const uint16_t *rank = nullptr;
    uint64_t pitch = 0;
    uint32_t rows = 0, n_samples = 0, beg = 0;
    const uint32_t *depth = nullptr;          // host [rows]
    const BvPileupToken *tokens = nullptr;    // host, sorted by (pos, sample)
    uint64_t n_tokens = 0;
    const uint8_t *d_text = nullptr;          // device: the tokens' text
    uint64_t text_bytes = 0;
};
void bv_pileup_view(const BvPileupState *t, BvPileupView *v);
// bv_pileup.hip's depth kernel over device ranks [rows][pitch]: depth[rows] and max_rank[rows] (device), queued on `st`
hipError_t bv_pileup_depth_launch(const uint16_t *rank, uint64_t pitch, uint32_t rows, uint32_t *depth, uint32_t *max_rank, hipStream_t st);
// The rows kept by the last bv_engine_text_submit, as they lie in device memory (bv_text.hip): false if there are none
struct BvKeptRows {
    const uint8_t *cell = nullptr, *phred = nullptr;  // [n_rows][pitch]
    uint64_t pitch = 0;
    uint32_t n_rows = 0, n_samples = 0;
};
bool bv_text_kept_rows(const BvTextState *t, BvKeptRows *rows);

// bv_engine_vcf_format's checks and pipeline (bv_vcf.hip) for lines whose heads and gt characters are not host bytes: `fill`
// queues on `st` the kernels that write gt [n_lines][4] and the heads, at head_off (given here on the host, from 0, and there
// on the device), where the copy of L->gt and L->head would have put them.  H == NULL: bv_engine_vcf_format itself.
struct BvVcfDeviceHeads {
    const uint64_t *head_off;  // host [n_lines + 1]
    int (*fill)(void *ctx, uint8_t *d_gt, uint8_t *d_head, const uint64_t *d_head_off, hipStream_t st);
    void *ctx;
};
struct bv_vcf_lines;
void bv_vcf_text_drop(bv_engine *e);  // the engine holds no formatted VCF text any more
int bv_vcf_format_lines(bv_engine *e, const char *who, const bv_vcf_lines *L, const BvVcfDeviceHeads *H, uint64_t *line_off, void *stream);

struct bv_engine {
    bv_engine_config cfg;
    hipStream_t stream = nullptr;      // engine-owned stream
    hipStream_t last_stream = nullptr; // stream of the last submit
    std::vector<hipStream_t> used_streams;  // every stream that carried work since the last bv_engine_wait
    hipEvent_t ev_host = nullptr;      // BV_FLAG_HOST_ORDERED: what the copy stream waits for before it reads host planes
    hipEvent_t ev_done = nullptr;      // end of the last submit: a submit on ANOTHER stream waits for it (shared scratch)
    bool ev_done_set = false;
    bool done_pending = false;         // the last submit's end is not recorded in ev_done yet (flush_done)
    hipStream_t done_stream = nullptr;
    uint32_t n_cu = 256;               // hipDeviceProp_t::multiProcessorCount
    int host_log_exact = 0;            // 1: the device replays shallow sites with the host libm's log(), verified bit-exact
    uint8_t *d_gid = nullptr;          // engine-owned copy of group_id, padded to 16 bytes with BV_NO_GROUP
    size_t d_gid_bytes = 0;
    BvTables *d_tables = nullptr;
    double *d_lnfact = nullptr;
    uint32_t *d_var_list = nullptr;
    // Counter blocks (BV_CTR_* words each, bv_kernels.h): every launch of launch_passes uses ONE block, the launches take the
    // blocks in turn (ctr_rot, below); everything else uses block 0.
    static constexpr uint32_t kCtrBlocks = 8;
    uint32_t *d_counters = nullptr;    // [kCtrBlocks][BV_CTR_WORDS]
    uint32_t *h_counters = nullptr;    // pinned host mirror
    uint32_t last_ctr_base = 0;        // the block the last launch used (its VARIANTS word is its variant count)
    // Submits take the counter blocks in turn (launch i: block i % kCtrBlocks): all blocks' per-launch lines are zeroed by ONE
    // 2-D fill every kCtrBlocks launches, and the host mirror is filled by bv_engine_wait, not by a copy behind every submit.
    // (Measured: the 23 KB device-to-host copy behind each submit kept the next submit's first kernel waiting ~10 us --
    // 100 k sites x 10 k samples 157.7 -> 160.4 M sites/s without it, 8,192-site batches 51.9 -> 55.7 M.)
    uint32_t ctr_rot = 0;
    bool ctr_mirror_stale = false;     // the device counters are ahead of h_counters
    static constexpr int kRing = 256;
    hipEvent_t ring[kRing][4] = {};    // per-submit events: start, end of pass 1, end of pass 2, [3] end of the streaming kernel of pass 1
    bool ring_one_kernel[kRing] = {};  // pass 1 was ONE kernel (long rows): [3] was not recorded, its time is [0] -> [1]
    int ring_head = 0, ring_count = 0; // pending (not yet accumulated) triplets
    int last_slot = -1;
    uint32_t n_launches = 0;           // launches since creation (BV_FLAG_SPARSE_TIMING times every eighth)
    uint32_t last_form = 0;            // BV_FORM_* bits of the last launch (bv_engine_last_launch_form)
    double acc1_ms = 0., acc2_ms = 0., acc_stream_ms = 0.;
    // short rows (bv_pass1_short.hip): HBM scratch between the streaming kernel and the solve kernel, an allocation each
    // (short_scratch in bv_engine_rows.hip: their order and bytes per site)
    BvSiteSummary *d_summ = nullptr;
    uint32_t *d_bins = nullptr, *d_cand_list = nullptr, *d_easy_list = nullptr, *d_easy3_list = nullptr, *d_ovf = nullptr;
    size_t short_bytes[6] = {};
    uint32_t *d_gitems = nullptr;      // pop-group calls handed from the pass-2 tally kernels to bv_p2g_solve16_kernel
    size_t d_gitems_bytes = 0;         // (items of BV_P2G_ITEM_WORDS words)
    uint8_t *d_gidp = nullptr;         // group ids prepared for bv_p2g_stream_kernel (bv_launch_gid_prepare)
    size_t d_gidp_bytes = 0;
    // more than BV_GROUPS_PER_ROUND pop-groups: pass 2 runs once per round of groups, on the round's own view of the group plane
    // (groups of other rounds read as "no group") and into records of its own, which are then moved to their columns of `gout`
    uint8_t *d_gid_round = nullptr;
    size_t d_gid_round_bytes = 0;
    bv_group_result *d_gout_round = nullptr;
    size_t d_gout_round_bytes = 0;
    BvChain *d_chain = nullptr;        // segment tables of chained launches (bv_engine_submit_many)
    uint8_t *d_ref_cat = nullptr;      // chained short-row launches: reference bases / records of all segments, contiguous
    bv_site_result *d_out_cat = nullptr;
    size_t d_chain_bytes = 0, d_ref_cat_bytes = 0, d_out_cat_bytes = 0;
    unsigned chain_next = 0;
    uint32_t acc_n = 0;
    bool submitted = false;
    // Host buffers (BV_MEM_HOST slabs, tiles, record buffers) go through a ring of device staging buffers filled by a
    // copy stream of their own: the PCIe copy of submit / tile k+1 runs under the kernels of k, and a buffer is reused
    // only after the work that read it has finished (events).
    static constexpr int kStage = 4;
    struct StageSlot {
        void *buf = nullptr;
        size_t bytes = 0;
        hipEvent_t copied = nullptr, freed = nullptr;
        hipStream_t cs = nullptr;  // the copy stream that fills this slot
        bool used = false;
    };
    StageSlot sring[kStage];
    unsigned sring_next = 0;
    hipStream_t copy_stream[2] = {nullptr, nullptr};  // alternate: the set-up of one copy hides under the transfer of the other
    // records of a host caller (stage_records): where the kernels write them, and where copy_records_back sends them
    bv_site_result *stage_out = nullptr;
    bv_group_result *stage_gout = nullptr;
    bv_site_result *host_out = nullptr;
    bv_group_result *host_gout = nullptr;
    size_t host_out_bytes = 0, host_gout_bytes = 0;
    // sample-axis tile mode (bv_engine_tiles.hip)
    struct TileJob {
        // the open job: bv_engine_tiles_begin resets it as a whole
        struct Job {
            bool open = false;
            bool join = false;         // joined rows (the planes of `rows`); else per-site tallies (`state`)
            bool ranks = false;
            uint32_t sites = 0, groups = 0, samples_total = 0, samples_seen = 0;
            uint32_t layout = 0;       // bv_slab.layout of the job's tiles (every tile of a job has the first one's)
            bool layout_set = false;
            bool filled = false;       // joined rows: the columns not yet delivered hold "uncovered" (a packed tile scatters into them)
            size_t pitch = 0, o_q = 0, o_mq = 0, o_rp = 0, o_gid = 0;  // joined rows: planes [sites][pitch] inside `rows`
            uint32_t stride = 0, rank_win = 1024, hg_off = 0, ord_off = 0;  // per-site tallies: the words of one site's state
        } job;
        // device buffers, kept from job to job and grown on demand (tile_job_free)
        uint8_t *rows = nullptr;       // joined-rows realisation: resident planes
        size_t rows_bytes = 0;
        uint32_t *state = nullptr, *maxr = nullptr;
        size_t state_bytes = 0, maxr_bytes = 0;
        uint32_t *ovf = nullptr;       // pool of read-position ranks beyond the window (bv_tiles.hip), kOvfCap entries
        static constexpr uint32_t kOvfCap = 1u << 22;
        // descriptor tables of the calls that take many tiles: a ring of pinned host + device buffers (desc_acquire / desc_send)
        static constexpr int kDescRing = 4;
        void *h_desc[kDescRing] = {}, *d_desc[kDescRing] = {};
        hipEvent_t ev_desc[kDescRing] = {};
        bool desc_used[kDescRing] = {};
        unsigned desc_next = 0;
    } tile;
    // BV_FLAG_LANES: device-resident submits alternate between two child engines (streams and scratch of their own), so that
    // the solve kernels of one submit run under the streaming kernels of the next; the parent runs no kernels then
    static constexpr int kMaxLanes = 4;
    bv_engine *lane[kMaxLanes] = {nullptr, nullptr, nullptr, nullptr};
    int n_lanes = 2;                   // (BASEVAR_AMD_LANES: tuning runs)
    unsigned lane_next = 0;
    int last_lane = -1;
    bool is_lane = false;
    hipEvent_t ev_entry = nullptr;     // what a lane waits for: the caller's stream at the time of the submit
    BvTextState *text = nullptr;       // created by the first bv_engine_text_parse
    BvBgzfState *bgzf = nullptr;       // created by the first bv_engine_bgzf_inflate
    BvDeflateState *deflate = nullptr;  // created by the first bv_engine_bgzf_deflate
    BvVcfState *vcf = nullptr;         // created by the first bv_engine_vcf_format
    BvPileupState *pileup = nullptr;   // created by the first bv_engine_pileup_set_reference
    BvPtextState *ptext = nullptr;     // created by the first bv_engine_pileup_text
    BvRtextState *rtext = nullptr;     // created by the first bv_engine_cvg_format / bv_engine_vcf_format_records
    BvIndelState *indel = nullptr;     // created by the first bv_engine_indel_tally
    BvTextTokState *ttok = nullptr;    // created by the first bv_engine_text_tokens_enable that turns the mode on
    mutable std::mutex mu;
    std::string err;
};

namespace bv_impl {
using StageSlot = bv_engine::StageSlot;

// sets bv_last_error(e) (or, without an engine, the global message) and returns `code`
int fail(bv_engine *e, int code, const std::string &msg);
#define BV_HIP(e, call)                                                                                  \
    do {                                                                                                 \
        hipError_t _s = (call);                                                                          \
        if (_s != hipSuccess)                                                                            \
            return ::bv_impl::fail((e), BV_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_s));  \
    } while (0)

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// e->text, e->bgzf, e->deflate, e->vcf, e->pileup, e->ptext: each is created by the first call that needs it, on the engine's device
template <class S>
S *engine_state(bv_engine *e, S *&state) {
    if (!state) {
        state = new S();
        state->device = e->cfg.device;
    }
    return state;
}

// A device buffer that only grows: at least `need` bytes behind *buf afterwards (hipFree synchronises with work that still uses it)
template <class T>
int grow_device(bv_engine *e, T **buf, size_t *bytes, size_t need) {
    if (need <= *bytes) return BV_OK;
    if (*buf) BV_HIP(e, hipFree(*buf));
    *buf = nullptr; *bytes = 0;
    BV_HIP(e, hipMalloc(buf, need));
    *bytes = need;
    return BV_OK;
}

// The same for scratch the caller can do with less of: an allocation that fails is no error, it leaves (NULL, 0)
template <class T>
int try_grow_device(bv_engine *e, T **buf, size_t *bytes, size_t need) {
    if (need <= *bytes) return BV_OK;
    if (*buf) BV_HIP(e, hipFree(*buf));
    *buf = nullptr; *bytes = 0;
    if (hipMalloc(buf, need) == hipSuccess) {
        *bytes = need;
    } else {
        (void)hipGetLastError();
        *buf = nullptr;
    }
    return BV_OK;
}

// ---- the indel tokens of parsed text rows (bv_text_tokens.hip), as the two parses of bv_text.hip drive them.  Each call does
// nothing while the mode is off (bv_engine_text_tokens_enable); the engine's device is selected.
struct BvTextTokRows {  // rows [row_first, row_first + n_rows) of the batch, whose text is on the device now
    const char *text;                   // byte k is text byte chunk_base + k
    const uint64_t *row_beg, *row_end;  // device [rows of the batch]: a row's first byte, and the byte behind its '\n'
    const uint8_t *rowflag;             // device: BV_TEXT_INDEL as bv_text_parse_kernel left it
    const uint32_t *foff;               // device [n_files]
    uint64_t chunk_base;
    uint32_t row_first, n_rows, n_files;
    // the rows of a parse job's add (bv_text_job.hip) of files [first_file, first_file + add_files): row_beg, row_end, row_first and
    // n_rows count the add's rows, add row p * add_files + k being row p * n_files + first_file + k of the batch.  add_files == 0: not so
    uint32_t first_file, add_files;
};
// ... and the store's device arrays, for the strided kernels of such an add (bv_text_job.hip), which bv_text_tokens_rows launches
// through these two: the count and the scan (base_* written from run_tok / run_txt on, totals[0 .. 2) the sums), and the write
struct BvTextTokStore {
    uint32_t *cnt_tok, *cnt_txt;            // [rows of the batch]
    uint64_t *base_tok, *base_txt, *totals;
    uint8_t *tok, *ttext;                   // descriptors (bv_pileup_token) and text
};
void text_job_tokens_count_scan(const BvTextTokRows &rows, const BvTextTokStore &s, uint64_t run_tok, uint64_t run_txt, hipStream_t st);
void text_job_tokens_write(const BvTextTokRows &rows, const BvTextTokStore &s, hipStream_t st);
int bv_text_tokens_begin(bv_engine *e, uint32_t P, uint32_t F, hipStream_t st);  // a parse begins: the last list is gone
int bv_text_tokens_rows(bv_engine *e, const BvTextTokRows &rows, hipStream_t st);  // behind the parse kernel of these rows; waits for `st`
int bv_text_tokens_finish(bv_engine *e, const uint8_t *pos_state, uint32_t P, uint32_t F, hipStream_t st);  // the positions' final states (host [P])
bool bv_text_tokens_on(const bv_engine *e);  // the mode is on
bool bv_text_tokens_stand(const bv_engine *e);  // the mode is on and the last parse's list stands (bv_engine_text_tokens would hand it out)

// ---- stream ordering (bv_engine.hip): work of one engine is serialised, whatever streams the caller alternates
int use_stream(bv_engine *e, hipStream_t st);  // before an entry point queues on `st`
int mark_done(bv_engine *e, hipStream_t st);   // what it queued on `st` is the end of the engine's work so far

// ---- the staging ring of host buffers (bv_engine.hip)
int stage_acquire(bv_engine *e, size_t bytes, StageSlot **out);
int stage_order(bv_engine *e, StageSlot *sl, hipStream_t st);
int stage_publish(bv_engine *e, StageSlot *sl, hipStream_t st);  // the copies are queued: `st` may read after them
int stage_release(bv_engine *e, StageSlot *sl, hipStream_t st);  // everything queued on `st` so far is the last reader
struct HostPlane {
    const void *src;     // host pointer (may be NULL: plane absent)
    size_t bytes;
    const uint8_t *dev;  // out: where the plane lives in the staging buffer
};
// Where `n` host planes go in a staging buffer: the bytes they take there, and whether they cross as ONE copy of [lo, hi)
struct HostPlanes {
    const uint8_t *lo = nullptr, *hi = nullptr;
    bool one_copy = false;
    size_t bytes = 0;
};
HostPlanes plan_host_planes(const HostPlane *pl, int n);
// Queue the copies of planes planned by plan_host_planes to `base` (device) on the copy stream `cs`; pl[i].dev = where plane i lands.
int copy_host_planes(bv_engine *e, HostPlane *pl, int n, const HostPlanes &h, uint8_t *base, hipStream_t cs);
// Queue the host->device copies of `n` planes into a fresh staging slot (+ `extra` bytes of device scratch behind them).
int stage_host_planes(bv_engine *e, HostPlane *pl, int n, size_t extra, StageSlot **slot_out, uint8_t **extra_dev, hipStream_t st);
// A host caller's planes and its [S] + [S][G] record buffers: the planes staged and published to `st`, device records behind them
// (*dout, *dgout) for the kernels to write, and `out` / `gout` remembered for copy_records_back
int stage_records(bv_engine *e, HostPlane *pl, int n, size_t S, size_t G, bv_site_result *out, bv_group_result *gout, StageSlot **slot,
                  bv_site_result **dout, bv_group_result **dgout, hipStream_t st);
int copy_records_back(bv_engine *e, hipStream_t st);  // (nothing for a device caller: e->host_out == NULL)

int stage_group_ids(bv_engine *e, const uint8_t *gid, uint32_t n_samples, bool host, hipStream_t st, const uint8_t **out);
int drain_timings(bv_engine *e, bool block);  // the pending event triplets -> the timing accumulators (bv_engine.hip)

// ---- the row path (bv_engine_rows.hip)
// One launch of the two passes: device-resident planes, and where the records go
struct RowLaunch {
    const uint8_t *bs = nullptr, *q = nullptr, *mq = nullptr;  // [n_sites][pitch]; mq NULL together with rp: no rank sums
    const uint16_t *rp = nullptr;
    const uint8_t *refb = nullptr;                             // [n_sites]
    const uint8_t *gid = nullptr;                              // [n_samples] padded (stage_group_ids), or NULL
    size_t pitch = 0;
    uint32_t n_sites = 0, n_samples = 0, n_groups = 0;
    uint32_t layout = 0;                                       // BV_SLAB_*
    bv_site_result *dout = nullptr;
    bv_group_result *dgout = nullptr;
    const BvChain *chain = nullptr;                            // device memory: a chained launch (planes per segment)
    bool chain_cat = false;                                    // chained short rows: refb / dout are the contiguous copies
};
// The two passes over device-resident planes + the copies back (records to a host caller, counters)
int launch_passes(bv_engine *e, const RowLaunch &L, hipStream_t st);
void row_scratch_free(bv_engine *e);        // bv_engine_destroy: the row path's grow-on-demand device buffers
void tile_job_free(bv_engine::TileJob &t);  // bv_engine_destroy: the tile mode's buffers (bv_engine_tiles.hip)
}  // namespace bv_impl
