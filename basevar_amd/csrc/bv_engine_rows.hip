// bv_engine_rows.hip -- row submits of the C ABI (include/basevar_amd.h): bv_engine_submit, bv_engine_submit_many(_g), and
// launch_passes, the two passes over device-resident planes that they and a joined-rows tile job (bv_engine_tiles.hip) end in.
//
// A submit is a check of its slab(s) (check_slab: nothing is queued before every slab has passed), the staging of what lives on
// the host, and one RowLaunch per launch.  launch_passes is a sequence of steps, each a function of this file; each kernel
// argument block is filled in one place from the RowLaunch and the engine.
#include <algorithm>
#include <array>
#include <string>

#include "bv_engine_impl.h"

using namespace bv_impl;

namespace {
#ifdef BV_TEAM_DEBUG
constexpr bool kRotateCounters = false;  // (the instrumented builds keep their stamps in the blocks behind the first)
#else
constexpr bool kRotateCounters = true;
#endif

// The group kernels hold one (base, phred) histogram per group in LDS and are built for at most BV_GROUPS_PER_ROUND of them;
// the reference takes any number of groups (a std::map, basetype_caller.cpp:372-410).  More groups run as ROUNDS of pass 2:
// round r sees groups [r x 32, r x 32 + 32) only (bv_launch_gid_round) and writes [S][32] records of its own, which one 2-D
// copy moves to their columns of the caller's [S][G] array.  Only round 0 forms the rank sums.
struct Rounds {
    size_t per, n;  // groups per round, rounds
};
Rounds rounds_of(size_t G) {
    const size_t per = G < BV_GROUPS_PER_ROUND ? G : (size_t)BV_GROUPS_PER_ROUND;
    return {per, G ? (G + per - 1) / per : 1};
}
size_t samples16(const RowLaunch &L) { return ((size_t)L.n_samples + 15) & ~(size_t)15; }
uint32_t rpr_tag(const RowLaunch &L) { return (L.layout & BV_SLAB_RPR_TAGGED) && L.rp != nullptr ? 1u : 0u; }
// whether the pop-group calls of the variant sites go through the item scratch (pop_group_scratch)
bool group_items(const bv_engine *e, const RowLaunch &L) { return L.n_groups && L.gid && L.dgout && !(e->cfg.flags & BV_FLAG_GROUP_INLINE); }

// ---- scratch: every buffer an allocation of its own, grown to the largest size seen
struct SiteScratch {
    void **buf;
    size_t per_site;
};
// short rows, between the kernels of pass 1: 48 B + 2 KiB + 28 B per site
std::array<SiteScratch, 6> short_scratch(bv_engine *e) {
    return {{{(void **)&e->d_summ, sizeof(BvSiteSummary)},
             {(void **)&e->d_bins, sizeof(uint32_t) * BV_S_BIN_STRIDE},
             {(void **)&e->d_cand_list, sizeof(uint32_t)},
             {(void **)&e->d_easy_list, sizeof(uint32_t)},
             {(void **)&e->d_easy3_list, sizeof(uint32_t)},
             {(void **)&e->d_ovf, sizeof(uint32_t) * 4}}};
}
int grow_short_scratch(bv_engine *e, uint32_t n_sites) {
    const auto sc = short_scratch(e);
    for (size_t i = 0; i < sc.size(); ++i) {
        const int rc = grow_device(e, sc[i].buf, &e->short_bytes[i], sc[i].per_site * (size_t)n_sites);
        if (rc != BV_OK) return rc;
    }
    return BV_OK;
}

// ---- the steps of launch_passes, in the order it takes them

// Per-pass timing: four event records per launch (start, end of the streaming kernel, end of pass 1, end of pass 2).  They are
// not free -- each is a packet the next kernel queues behind: ~15 us per launch together (measured: 100 k sites x 10 k samples
// 158.4 -> 162.4 M sites/s without them, 8,192-site batches 56.7 -> 63.0 M) -- so BV_FLAG_SPARSE_TIMING records them for one
// launch in eight; the averages of bv_engine_timing_get then rest on those launches.  *ev: this launch's events, NULL untimed.
int timing_slot(bv_engine *e, hipEvent_t **ev) {
    const bool timed = !(e->cfg.flags & BV_FLAG_SPARSE_TIMING) || (e->n_launches % 8u) == 0u;
    e->n_launches += 1;
    *ev = nullptr;
    if (!timed) return BV_OK;
    if (e->ring_count == bv_engine::kRing) {
        int rc = drain_timings(e, true);  // ring full: fold the oldest submits first
        if (rc != BV_OK) return rc;
    }
    const int slot = e->ring_head;
    e->ring_head = (e->ring_head + 1) % bv_engine::kRing;
    e->ring_count += 1;
    e->last_slot = slot;
    *ev = e->ring[slot];
    e->ring_one_kernel[slot] = false;
    return BV_OK;
}

// Scratch for the group calls of the variant sites (1.5 KiB per site x group), grown on demand and capped at 8 GiB: the variant
// sites past the cap keep the one-wave-per-group solver inside the tally kernel.  An allocation that fails is retried at half
// the size (the inline path takes what the scratch cannot).  And the group plane as the perm-form tallies read it (short rows:
// bv_p2g_stream_kernel; long rows: bv_p2_fast_sweep) -- several rounds of groups: prepared per round, by pass2_rounds.
int pop_group_scratch(bv_engine *e, const RowLaunch &L, const Rounds &rd, hipStream_t st) {
    if (!group_items(e, L)) return BV_OK;
    const size_t item = sizeof(uint32_t) * BV_P2G_ITEM_WORDS;
    const uint64_t want64 = (uint64_t)L.n_sites * rd.per, most = (8192ull << 20) / item;
    for (size_t want = (size_t)(want64 < most ? want64 : most);; want /= 2u) {
        const int rc = try_grow_device(e, &e->d_gitems, &e->d_gitems_bytes, item * want);
        if (rc != BV_OK) return rc;
        if (e->d_gitems || want < 1024u) break;  // (nothing at all: every group is solved inside the tally kernel)
    }
    const int rc = grow_device(e, &e->d_gidp, &e->d_gidp_bytes, samples16(L) + 256);
    if (rc != BV_OK) return rc;
    if (rd.n == 1) {
        bv_launch_gid_prepare(L.gid, e->d_gidp, (uint32_t)samples16(L), L.n_groups, st);
        BV_HIP(e, hipGetLastError());
    }
    return BV_OK;
}

// Submits take the counter blocks in turn (bv_engine::ctr_rot).  *ctr: this launch's block, its per-launch lines zero.
int counter_block(bv_engine *e, hipStream_t st, uint32_t **ctr) {
    uint32_t cb = 0;
    if (kRotateCounters) {
        cb = e->ctr_rot % bv_engine::kCtrBlocks;
        if (cb == 0)  // a new round: the per-launch lines of every block (not the sticky error counters behind them) in one fill
            BV_HIP(e, hipMemset2DAsync(e->d_counters, sizeof(uint32_t) * BV_CTR_WORDS, 0, sizeof(uint32_t) * BV_CTR_PER_LAUNCH * BV_CTR_STRIDE,
                                       bv_engine::kCtrBlocks, st));
        e->ctr_rot += 1;
    } else {
        e->ctr_rot = 0;  // (the next rotating launch starts a round of its own)
        BV_HIP(e, hipMemsetAsync(e->d_counters, 0, sizeof(uint32_t) * BV_CTR_PER_LAUNCH * BV_CTR_STRIDE, st));
    }
    e->last_ctr_base = cb;
    *ctr = e->d_counters + (size_t)cb * BV_CTR_WORDS;
    return BV_OK;
}

// Pass 1 of rows of at most BV_SHORT_ROW_MAX samples.  *pass2_fused: its kernel has streamed the pass-2 rows too.
//
// Rows of at least three 4 KiB slots: pass 1 as ONE persistent kernel (bv_pass1_fused.hip: solver waves beside the streaming
// waves of every workgroup), which streams the variant sites' rank-sum rows (pass 2) too -- with pop-groups of any number: the
// launch behind then carries the group tallies only (the rank sums of a variant row cost this kernel 0.12 ms per 100 k sites,
// the workgroup-per-row group kernel 0.16-0.2).  Shorter rows, and BV_FLAG_SHORT_ROW_FORM(9) (tests: an independent
// realisation): a streaming kernel, a solve kernel, pass 2 a launch of its own (bv_pass1_short.hip);
// BV_FLAG_SHORT_ROW_FORM(10): the fused kernel for pass 1 only.
int pass1_short_rows(bv_engine *e, const RowLaunch &L, uint32_t *ctr, hipEvent_t *ev, hipStream_t st, bool *pass2_fused) {
    const int rc = grow_short_scratch(e, L.n_sites);
    if (rc != BV_OK) return rc;
    BvP1ShortArgs s1;
    s1.bs = L.bs; s1.q = L.q; s1.ref_base = L.refb; s1.pitch = L.pitch; s1.n_sites = L.n_sites; s1.n_samples = L.n_samples;
    s1.flags = e->cfg.flags; s1.n_cu = e->n_cu; s1.min_af = e->cfg.min_af; s1.tables = e->d_tables; s1.out = L.dout;
    s1.var_list = e->d_var_list; s1.counters = ctr;
    s1.summ = e->d_summ; s1.bins = e->d_bins;
    s1.cand_list = e->d_cand_list; s1.easy_list = e->d_easy_list; s1.easy3_list = e->d_easy3_list;
    s1.ovf = e->d_ovf;
    s1.ch = L.chain;
    s1.mapq = nullptr; s1.rpr = nullptr; s1.rpr_tag = rpr_tag(L);
    const uint32_t form = (e->cfg.flags >> 12) & 0xFu;
    if (form != 9u && bv_p1s_fused_takes(s1)) {
        if (ev) e->ring_one_kernel[e->last_slot] = true;
        if (form != 10u && L.mq != nullptr && L.rp != nullptr && !(e->cfg.flags & BV_FLAG_PASS2_SWEEP)) {
            s1.mapq = L.mq; s1.rpr = L.rp;
            *pass2_fused = true;
        }
        bv_launch_p1s_fused(s1, st);
        BV_HIP(e, hipGetLastError());
        e->last_form |= BV_FORM_ONE_KERNEL | (*pass2_fused ? BV_FORM_PASS2_FUSED : 0u);
    } else {
        bv_launch_p1s_stream(s1, st);
        BV_HIP(e, hipGetLastError());
        if (ev) BV_HIP(e, hipEventRecord(ev[3], st));
        bv_launch_p1s_solve(s1, st);
        BV_HIP(e, hipGetLastError());
    }
    if (ev) BV_HIP(e, hipEventRecord(ev[1], st));
    return BV_OK;
}

// Pass 1 of longer rows: one kernel (bv_pass1.hip), no separate event for "the streaming kernel"
int pass1_long_rows(bv_engine *e, const RowLaunch &L, uint32_t *ctr, hipEvent_t *ev, hipStream_t st) {
    if (ev) e->ring_one_kernel[e->last_slot] = true;
    BvPass1Args a1;
    a1.bs = L.bs; a1.q = L.q; a1.ref_base = L.refb; a1.pitch = L.pitch; a1.n_sites = L.n_sites;
    a1.n_samples = L.n_samples; a1.flags = e->cfg.flags; a1.min_af = e->cfg.min_af; a1.tables = e->d_tables; a1.out = L.dout;
    a1.var_list = e->d_var_list; a1.counters = ctr; a1.n_cu = e->n_cu;
    a1.ch = L.chain;
    bv_launch_pass1(a1, st);
    BV_HIP(e, hipGetLastError());
    e->last_form |= BV_FORM_ONE_KERNEL;
    if (ev) BV_HIP(e, hipEventRecord(ev[1], st));
    return BV_OK;
}

// Pass 2, once per round of groups (one round unless there are more than BV_GROUPS_PER_ROUND): a round beyond the only one
// runs on its own view of the group plane and into records of its own (bv_engine::d_gid_round, d_gout_round)
int pass2_rounds(bv_engine *e, const RowLaunch &L, const Rounds &rd, uint32_t *ctr, bool pass2_fused, hipStream_t st) {
    const size_t S = L.n_sites, G = L.n_groups;
    const bool items = group_items(e, L);
    BvPass2Args a2;
    a2.bs = L.bs; a2.q = L.q; a2.mapq = L.mq; a2.rpr = L.rp; a2.ref_base = L.refb; a2.group_id = L.gid; a2.pitch = L.pitch;
    a2.n_sites = L.n_sites; a2.n_samples = L.n_samples; a2.n_groups = L.n_groups;
    a2.min_af = e->cfg.min_af; a2.tables = e->d_tables; a2.out = L.dout; a2.gout = L.dgout;
    a2.var_list = e->d_var_list; a2.counters = ctr; a2.n_cu = e->n_cu; a2.flags = e->cfg.flags;
    a2.gitems = items ? e->d_gitems : nullptr;
    a2.gitem_cap = items ? (uint32_t)(e->d_gitems_bytes / (sizeof(uint32_t) * BV_P2G_ITEM_WORDS)) : 0u;
    a2.gidp = items ? e->d_gidp : nullptr;
    a2.ch = L.chain;
    a2.ch_cat = L.chain_cat ? 1u : 0u;
    a2.rpr_tag = rpr_tag(L);
    for (size_t r = 0; r < rd.n; ++r) {
        const size_t g_lo = r * rd.per, g_n = rd.n > 1 ? std::min(rd.per, G - g_lo) : G;  // this round's groups
        BvPass2Args ac = a2;
        if (rd.n > 1) {
            bv_launch_gid_round(L.gid, e->d_gid_round, (uint32_t)samples16(L), (uint32_t)g_lo, (uint32_t)g_n, st);
            BV_HIP(e, hipGetLastError());
            bv_launch_gid_prepare(e->d_gid_round, e->d_gidp, (uint32_t)samples16(L), (uint32_t)g_n, st);
            BV_HIP(e, hipGetLastError());
            BV_HIP(e, hipMemsetAsync(e->d_gout_round, 0, S * g_n * sizeof(bv_group_result), st));
            ac.group_id = e->d_gid_round; ac.n_groups = (uint32_t)g_n; ac.gout = e->d_gout_round;
        }
        if (pass2_fused || r > 0) {  // the rank sums are formed already (by pass 1's kernel / by round 0): what is left is the pop-groups
            if (G == 0) continue;
            ac.mapq = nullptr; ac.rpr = nullptr;
        }
        bv_launch_pass2(ac, st);
        BV_HIP(e, hipGetLastError());
        bv_launch_p2g_solve16(ac, st);
        BV_HIP(e, hipGetLastError());
        if (rd.n > 1)  // the round's records -> columns [g_lo, g_lo + g_n) of every site's groups
            BV_HIP(e, hipMemcpy2DAsync(L.dgout + g_lo, G * sizeof(bv_group_result), e->d_gout_round, g_n * sizeof(bv_group_result),
                                       g_n * sizeof(bv_group_result), S, hipMemcpyDeviceToDevice, st));
    }
    return BV_OK;
}
}  // namespace

void bv_impl::row_scratch_free(bv_engine *e) {
    for (const SiteScratch &s : short_scratch(e))
        if (*s.buf) (void)hipFree(*s.buf);
    void *const rest[] = {e->d_gitems, e->d_gidp, e->d_gid_round, e->d_gout_round, e->d_chain, e->d_ref_cat, e->d_out_cat};
    for (void *p : rest)
        if (p) (void)hipFree(p);
}

// The two passes over device-resident planes + the copies back (records to a host caller, counters).
//
// (Round 3 also ran short-row batches as a software pipeline of chunks over two streams -- the solve kernels of chunk c under the
// streaming kernel of chunk c + 1.  Measured a loss at every size (beside a streaming kernel the solve kernels get one
// workgroup per CU and run 3 x longer, the streaming kernel slows by 50-70 %): removed; docs/history/DESIGN_round3.md 4.2b.)
int bv_impl::launch_passes(bv_engine *e, const RowLaunch &L, hipStream_t st) {
    const size_t S = L.n_sites, G = L.n_groups;
    const Rounds rd = rounds_of(G);
    if (rd.n > 1 && L.chain != nullptr) return fail(e, BV_ERR_INVALID_ARG, "launch_passes: more than 32 pop-groups do not chain");
    if (G && L.chain == nullptr) BV_HIP(e, hipMemsetAsync(L.dgout, 0, S * G * sizeof(bv_group_result), st));  // (chained: per segment, by the caller)
    if (rd.n > 1) {
        int rc = grow_device(e, &e->d_gid_round, &e->d_gid_round_bytes, up256(L.n_samples) + 256);
        if (rc == BV_OK) rc = grow_device(e, &e->d_gout_round, &e->d_gout_round_bytes, S * rd.per * sizeof(bv_group_result));
        if (rc != BV_OK) return rc;
    }
    hipEvent_t *ev = nullptr;
    uint32_t *ctr = nullptr;
    int rc = timing_slot(e, &ev);
    if (rc == BV_OK) rc = pop_group_scratch(e, L, rd, st);
    if (rc == BV_OK) rc = counter_block(e, st, &ctr);
    if (rc != BV_OK) return rc;
    // Rows of at most BV_SHORT_ROW_MAX samples take the short-row forms of pass 1 (bv_pass1_fused.hip; bv_pass1_short.hip)
    const bool short_rows = L.n_samples <= BV_SHORT_ROW_MAX;
    bool pass2_fused = false;
    e->last_form = short_rows ? BV_FORM_SHORT_ROWS : 0u;
    if (ev) BV_HIP(e, hipEventRecord(ev[0], st));
    rc = short_rows ? pass1_short_rows(e, L, ctr, ev, st, &pass2_fused) : pass1_long_rows(e, L, ctr, ev, st);
    if (rc == BV_OK) rc = pass2_rounds(e, L, rd, ctr, pass2_fused, st);
    if (rc != BV_OK) return rc;
    if (ev) BV_HIP(e, hipEventRecord(ev[2], st));

    if (kRotateCounters) e->ctr_mirror_stale = true;  // mirrored by bv_engine_wait
    else BV_HIP(e, hipMemcpyAsync(e->h_counters, e->d_counters, sizeof(uint32_t) * BV_CTR_WORDS * bv_engine::kCtrBlocks, hipMemcpyDeviceToHost, st));
    rc = copy_records_back(e, st);
    if (rc != BV_OK) return rc;
    e->submitted = true;
    return mark_done(e, st);
}

namespace {
// ---- the checks of a slab and its record buffers: the error code and why the engine refuses them, or why == NULL.  The entry
// points put their own name (and the slab's number) in front.
struct SlabCheck {
    int code;
    const char *why;
};
// (the one reason that bv_engine_submit_many words differently, where it was given no gouts array at all)
const char kGroupsNeedGout[] = "n_groups > 0 needs group_id and gout";
SlabCheck check_slab(const bv_engine *e, const bv_slab *slab, const bv_site_result *out, const bv_group_result *gout) {
    auto misaligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; };
    const int bad = BV_ERR_INVALID_ARG;
    if (!slab || !out) return {bad, "null slab/out"};
    if (slab->n_sites == 0) return {bad, "n_sites == 0"};
    if (slab->n_sites > e->cfg.max_sites) return {BV_ERR_TOO_LARGE, "n_sites exceeds cfg.max_sites"};
    if (slab->n_samples == 0 || slab->pitch < slab->n_samples || (slab->pitch & 15ull)) return {bad, "pitch must be >= n_samples and a multiple of 16"};
    if (!slab->base_strand || !slab->qual || !slab->ref_base) return {bad, "base_strand, qual and ref_base planes are required"};
    if ((slab->mapq == nullptr) != (slab->rpr == nullptr)) return {bad, "mapq and rpr planes must be given together"};
    if (slab->n_groups > BV_MAX_GROUPS) return {bad, "n_groups exceeds BV_MAX_GROUPS"};
    if (slab->n_groups > 0 && (!slab->group_id || !gout)) return {bad, kGroupsNeedGout};
    if (misaligned(slab->base_strand) || misaligned(slab->qual) || misaligned(slab->mapq) || misaligned(slab->rpr))
        return {bad, "planes must be 16-byte aligned"};
    if (slab->mem_kind != BV_MEM_HOST && misaligned(out)) return {bad, "device record buffers must be 16-byte aligned"};
    if ((slab->layout & ~BV_SLAB_RPR_TAGGED) || slab->reserved_) return {bad, "unknown bv_slab.layout bits (built against another BV_ABI_VERSION?)"};
    return {BV_OK, nullptr};
}

// BV_FLAG_LANES: a device-resident submit goes to the child engine whose turn it is, on that child's own stream, ordered behind
// what the caller's stream holds now; the caller's stream gets nothing back (bv_engine_join / bv_engine_wait)
int submit_to_lane(bv_engine *e, const bv_slab *slab, bv_site_result *out, bv_group_result *gout, void *stream_) {
    const int k = (int)(e->lane_next++ % (unsigned)e->n_lanes);
    if (!e->lane[k]) {
        bv_engine_config c = e->cfg;
        c.flags &= ~BV_FLAG_LANES;
        int rc = bv_engine_create(&c, &e->lane[k]);
        if (rc != BV_OK) return fail(e, rc, std::string("bv_engine_submit: lane engine: ") + bv_last_error(nullptr));
        e->lane[k]->is_lane = true;
    }
    bv_engine *l = e->lane[k];
    // (only if that stream holds unfinished work: recording an event on an idle stream and waiting for it on another cost
    // 0.5-2 ms per submit on this stack -- measured, round 3 -- against ~10 us when the marker follows real work)
    // NULL means the engine's own stream here too (include/basevar_amd.h): planes written on bv_engine_stream(e) just
    // before a NULL-stream submit are ordered like those of any other stream.  (A stream that is being captured
    // answers the query with an error: treated as "holds work", the marker is then part of the capture.)
    hipStream_t src = stream_ ? (hipStream_t)stream_ : e->stream;
    if (hipStreamQuery(src) != hipSuccess) {
        (void)hipGetLastError();  // hipErrorNotReady is the answer, not an error
        if (!e->ev_entry) BV_HIP(e, hipEventCreateWithFlags(&e->ev_entry, hipEventDisableTiming));
        BV_HIP(e, hipEventRecord(e->ev_entry, src));
        BV_HIP(e, hipStreamWaitEvent(l->stream, e->ev_entry, 0));
    }
    const int rc = bv_engine_submit(l, slab, out, gout, nullptr);
    if (rc != BV_OK) return fail(e, rc, bv_last_error(l));
    e->last_lane = k;
    e->submitted = true;
    return BV_OK;
}
}  // namespace

extern "C" {

int bv_engine_submit(bv_engine *e, const bv_slab *slab, bv_site_result *out, bv_group_result *gout, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_submit: null engine");
    const SlabCheck c = check_slab(e, slab, out, gout);
    if (c.why) return fail(e, c.code, std::string("bv_engine_submit: ") + c.why);

    BV_HIP(e, hipSetDevice(e->cfg.device));
    if ((e->cfg.flags & BV_FLAG_LANES) && !e->is_lane && slab->mem_kind != BV_MEM_HOST) return submit_to_lane(e, slab, out, gout, stream_);
    e->last_lane = -1;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    {
        int rc = use_stream(e, st);
        if (rc != BV_OK) return rc;
    }

    RowLaunch L;
    L.bs = slab->base_strand; L.q = slab->qual; L.mq = slab->mapq; L.rp = slab->rpr; L.refb = slab->ref_base; L.gid = slab->group_id;
    L.pitch = slab->pitch; L.n_sites = slab->n_sites; L.n_samples = slab->n_samples; L.n_groups = slab->n_groups; L.layout = slab->layout;
    L.dout = out; L.dgout = gout;
    const size_t S = slab->n_sites, P = slab->pitch, G = slab->n_groups;
    StageSlot *slot = nullptr;
    if (slab->mem_kind == BV_MEM_HOST) {
        // host planes -> a staging slot, copied by the copy stream (under the kernels of the previous submit)
        HostPlane pl[5] = {{L.bs, S * P, nullptr}, {L.q, S * P, nullptr}, {L.mq, L.mq ? S * P : 0, nullptr},
                           {L.rp, L.rp ? S * P * 2 : 0, nullptr}, {L.refb, S, nullptr}};
        const int rc = stage_records(e, pl, 5, S, G, out, gout, &slot, &L.dout, &L.dgout, st);
        if (rc != BV_OK) return rc;
        L.bs = pl[0].dev; L.q = pl[1].dev; L.mq = pl[2].dev;
        L.rp = reinterpret_cast<const uint16_t *>(pl[3].dev);
        L.refb = pl[4].dev;
    } else {
        e->host_out = nullptr; e->host_gout = nullptr;
    }
    if (G) {
        int rc = stage_group_ids(e, slab->group_id, slab->n_samples, slab->mem_kind == BV_MEM_HOST, st, &L.gid);
        if (rc != BV_OK) return rc;
    }

    int rc = launch_passes(e, L, st);
    if (rc == BV_OK && slot) rc = stage_release(e, slot, st);  // planes read, records copied back: the slot may be refilled
    return rc;
}

// Several device-resident slabs of one row length, ONE launch per pass (BvChain): what a host with a few small batches
// ready should call -- the tail of every batch but the last hides under the next batch's stream.  Falls back to one
// submit per slab whenever the chained kernels do not apply (short rows, pop-groups, host memory, a forced kernel shape).
int bv_engine_submit_many(bv_engine *e, uint32_t n_slabs, const bv_slab *slabs, bv_site_result *const *outs, void *stream_) {
    return bv_engine_submit_many_g(e, n_slabs, slabs, outs, nullptr, stream_);
}

// The same with pop-groups: gouts[k] = slab k's [n_sites][n_groups] records (NULL array: no slab may have groups).  A queue
// with groups chains when every slab names the SAME group_id array and group count (one cohort).
int bv_engine_submit_many_g(bv_engine *e, uint32_t n_slabs, const bv_slab *slabs, bv_site_result *const *outs,
                            bv_group_result *const *gouts, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_submit_many: null engine");
    if (!slabs || !outs || n_slabs == 0) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_submit_many: null / empty argument");
    bool chainable = n_slabs > 1;
    uint64_t total = 0;
    // every slab is checked before anything is launched
    for (uint32_t k = 0; k < n_slabs; ++k) {
        const bv_slab &s = slabs[k];
        const SlabCheck c = check_slab(e, &s, outs[k], gouts ? gouts[k] : nullptr);
        if (c.why == kGroupsNeedGout && !gouts && s.group_id)
            return fail(e, c.code, "bv_engine_submit_many: a slab with pop-groups needs group_id and its gouts[k] (bv_engine_submit_many_g)");
        if (c.why) return fail(e, c.code, "bv_engine_submit_many: slab " + std::to_string(k) + ": " + c.why);
        // (host memory and the diagnostic kernel choices take kernels that know no chain; a queue is one cohort: one row
        // length, one pitch, one set of planes, one group assignment)
        chainable = chainable && s.mem_kind != BV_MEM_HOST && !(e->cfg.flags & (BV_FLAG_PASS2_SWEEP | BV_FLAG_GROUP_INLINE)) &&
                    s.n_samples == slabs[0].n_samples && s.pitch == slabs[0].pitch && (s.mapq == nullptr) == (slabs[0].mapq == nullptr) &&
                    s.n_groups == slabs[0].n_groups && (s.n_groups == 0 || s.group_id == slabs[0].group_id) && s.layout == slabs[0].layout;
        total += s.n_sites;
    }
    const uint32_t G = slabs[0].n_groups;
    // pop-groups chain only when every (site, group) of a launch has an item in the scratch (no inline solves: their kernels
    // would need the segment look-up too) -- checked per launch below through the 8 GiB cap of launch_passes
    if (chainable && G && (uint64_t)std::min<uint64_t>(total, e->cfg.max_sites) * G * sizeof(uint32_t) * BV_P2G_ITEM_WORDS > (8192ull << 20)) chainable = false;
    if (G > BV_GROUPS_PER_ROUND) chainable = false;  // several rounds of groups (launch_passes): slab by slab
    if (!chainable) {
        for (uint32_t k = 0; k < n_slabs; ++k) {
            int rc = bv_engine_submit(e, &slabs[k], outs[k], slabs[k].n_groups ? gouts[k] : nullptr, stream_);
            if (rc != BV_OK) return rc;
        }
        return BV_OK;
    }
    if (total > e->cfg.max_sites) return fail(e, BV_ERR_TOO_LARGE, "bv_engine_submit_many: the slabs together exceed cfg.max_sites");
    BV_HIP(e, hipSetDevice(e->cfg.device));
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    {
        int rc = use_stream(e, st);
        if (rc != BV_OK) return rc;
    }
    e->host_out = nullptr; e->host_gout = nullptr;
    e->last_lane = -1;
    const size_t P = slabs[0].pitch;
    const bool ranks = slabs[0].mapq != nullptr;
    const uint8_t *gid = nullptr;
    if (G) {
        int rc = stage_group_ids(e, slabs[0].group_id, slabs[0].n_samples, false, st, &gid);
        if (rc != BV_OK) return rc;
    }
    // at most BV_MAX_CHAIN slabs per launch
    for (uint32_t k0 = 0; k0 < n_slabs; k0 += BV_MAX_CHAIN) {
        const uint32_t nk = n_slabs - k0 < (uint32_t)BV_MAX_CHAIN ? n_slabs - k0 : (uint32_t)BV_MAX_CHAIN;
        BvChain ch{};
        ch.n = nk;
        uint32_t first = 0;
        for (uint32_t i = 0; i < nk; ++i) {
            const bv_slab &s = slabs[k0 + i];
            const size_t bias = (size_t)first * P;
            ch.first[i] = first;
            ch.bs[i] = s.base_strand - bias; ch.q[i] = s.qual - bias;
            ch.mapq[i] = ranks ? s.mapq - bias : nullptr; ch.rpr[i] = ranks ? s.rpr - bias : nullptr;
            ch.ref_base[i] = s.ref_base - first;
            ch.out[i] = outs[k0 + i] - first;
            ch.gout[i] = G ? gouts[k0 + i] - (size_t)first * G : nullptr;
            if (G) BV_HIP(e, hipMemsetAsync(gouts[k0 + i], 0, (size_t)s.n_sites * G * sizeof(bv_group_result), st));
            first += s.n_sites;
        }
        // the launch's sites are the segments' together; of one slab (nk == 1), or chained with long rows -- where every kernel
        // looks its segment up per site (planes, reference bases, records) --, the first slab's pointers stand for the rest
        const bv_slab &s0 = slabs[k0];
        RowLaunch L;
        L.bs = s0.base_strand; L.q = s0.qual; L.mq = s0.mapq; L.rp = s0.rpr; L.refb = s0.ref_base; L.gid = gid;
        L.pitch = P; L.n_sites = first; L.n_samples = s0.n_samples; L.n_groups = G; L.layout = s0.layout;
        L.dout = outs[k0]; L.dgout = G ? gouts[k0] : nullptr;
        if (nk > 1) {
            // the segment table lives in device memory (a ring of 16: a table is rewritten only 16 chained launches later)
            int rc = grow_device(e, &e->d_chain, &e->d_chain_bytes, sizeof(BvChain) * 16);
            if (rc != BV_OK) return rc;
            BvChain *d_ch = e->d_chain + (e->chain_next++ & 15u);
            BV_HIP(e, hipMemcpyAsync(d_ch, &ch, sizeof(BvChain), hipMemcpyHostToDevice, st));
            L.chain = d_ch;
        }
        if (nk == 1 || s0.n_samples > BV_SHORT_ROW_MAX) {
            int rc = launch_passes(e, L, st);
            if (rc != BV_OK) return rc;
            continue;
        }
        // chained short rows: the planes are looked up per row (wave-uniform places only); the per-site reference bases and records,
        // which the lane-per-site and four-per-wave kernels touch with one site per lane, go through contiguous copies
        // (the pop-group records are written once per (variant site, group): looked up where they are written)
        int rc = grow_device(e, &e->d_ref_cat, &e->d_ref_cat_bytes, (size_t)e->cfg.max_sites + 256);
        if (rc == BV_OK) rc = grow_device(e, &e->d_out_cat, &e->d_out_cat_bytes, sizeof(bv_site_result) * (size_t)e->cfg.max_sites);
        if (rc != BV_OK) return rc;
        bv_launch_chain_gather_ref(L.chain, first, e->d_ref_cat, st);
        BV_HIP(e, hipGetLastError());
        L.refb = e->d_ref_cat; L.dout = e->d_out_cat; L.chain_cat = true;
        rc = launch_passes(e, L, st);
        if (rc != BV_OK) return rc;
        bv_launch_chain_scatter_out(L.chain, first, e->d_out_cat, st);
        BV_HIP(e, hipGetLastError());
        rc = mark_done(e, st);  // the scatter is the end of this submit
        if (rc != BV_OK) return rc;
    }
    return BV_OK;
}

}  // extern "C"
