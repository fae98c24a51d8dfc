// bv_engine_tiles.hip -- the sample-axis tile mode of the C ABI (include/basevar_amd.h): a job of n_sites rows arrives as
// tiles of columns (bv_engine_tiles_begin / _add* ... / _finish), dense or packed, one tile or many per call.
//
// Two realisations behind one protocol: JOINED ROWS -- the tiles are moved to their columns of [n_sites][pitch] planes
// resident in HBM and the job finishes as one launch_passes (bv_engine_rows.hip) over them -- and, where those planes do not fit or
// BV_FLAG_TILE_STATE asks for it, PER-SITE TALLIES that every tile adds to (bv_tiles.hip).  Every add call is a check of its
// tiles (check_*_tile: nothing changes before every tile of the call has passed) and then one of four ways to launch.
#include <algorithm>
#include <cstring>

#include "bv_engine_impl.h"

using namespace bv_impl;

namespace {
using Job = bv_engine::TileJob::Job;

// what every entry point does before it queues anything: the device, the caller's stream (NULL: the engine's), ordered
int job_stream(bv_engine *e, void *stream_, hipStream_t *st) {
    BV_HIP(e, hipSetDevice(e->cfg.device));
    *st = stream_ ? (hipStream_t)stream_ : e->stream;
    return use_stream(e, *st);
}

uint32_t rpr_tag(const Job &j) { return (j.layout & BV_SLAB_RPR_TAGGED) ? 1u : 0u; }

// ---- the checks of a tile: why the open job refuses it, or NULL.  `seen`: samples delivered before this tile (the job's and the
// call's earlier tiles'), `layout0`: the layout of the call's first tile.  The entry points put their own name in front.
const char *check_dense_tile(const bv_engine *e, const bv_slab &t, uint64_t seen, uint32_t layout0) {
    const Job &j = e->tile.job;
    if (t.n_sites != j.sites) return "tile n_sites differs from the job's";
    if (t.n_samples == 0 || t.pitch < t.n_samples || (t.pitch & 15ull) || !t.base_strand || !t.qual) return "bad tile geometry or missing planes";
    if (j.ranks && (!t.mapq || !t.rpr)) return "job was opened with rank planes";
    if (j.groups && !t.group_id) return "job has groups, tile has no group_id";
    if (seen + t.n_samples > j.samples_total) return "more samples than announced";
    if ((t.layout & ~BV_SLAB_RPR_TAGGED) || t.reserved_ || t.layout != layout0 || (j.layout_set && t.layout != j.layout))
        return "every tile of a job must have the same bv_slab.layout (known bits only)";
    return nullptr;
}

// (the one reason that bv_engine_tiles_add_sparse words differently: "tile n_sites ..." where the _many form says "tile k: n_sites ...")
const char kSparseSitesDiffer[] = "n_sites differs from the job's";
const char *check_sparse_tile(const bv_engine *e, const bv_sparse_tile &t, uint64_t seen, uint32_t layout0) {
    const Job &j = e->tile.job;
    if (t.n_sites != j.sites) return kSparseSitesDiffer;
    if (t.n_samples == 0 || t.n_samples > 65536u || !t.row_start || (t.n_entries && (!t.sample || !t.base_strand || !t.qual)))
        return "bad tile geometry (at most 65,536 samples per tile) or missing arrays";
    if (j.ranks && t.n_entries && (!t.mapq || !t.rpr)) return "job was opened with rank planes";
    if (j.groups && !t.group_id) return "job has groups, tile has no group_id";
    if (seen + t.n_samples > j.samples_total) return "more samples than announced";
    if ((t.layout & ~BV_SLAB_RPR_TAGGED) || t.layout != layout0 || (j.layout_set && t.layout != j.layout))
        return "every tile of a job must have the same layout (known bits only)";
    if (t.mem_kind == BV_MEM_HOST) {  // the kernels trust row_start: on the host it costs a pass over n_sites + 1 words
        const uint32_t *rs = t.row_start;
        bool ok = rs[0] == 0 && rs[t.n_sites] == t.n_entries;
        for (uint32_t s = 0; s < t.n_sites && ok; ++s) ok = rs[s] <= rs[s + 1];
        if (!ok) return "row_start must start at 0, never decrease and end at n_entries";
    }
    return nullptr;
}

// ---- the descriptor ring: one table of kDescBytes per call group, written in pinned memory and copied on the caller's stream
constexpr size_t kDescBytes = sizeof(BvTileScatterPlane) * 5 * BV_TILE_MANY_MAX;  // five planes of BV_TILE_MANY_MAX dense tiles
static_assert(sizeof(BvSparseTileDesc) * BV_TILE_MANY_MAX <= kDescBytes, "a group's packed-tile descriptors must fit one table of the ring");
// the ring's next table: *h (pinned host) is the caller's to fill once this returns, *d is where desc_send puts it
int desc_acquire(bv_engine *e, int *slot, void **h, void **d) {
    bv_engine::TileJob &t = e->tile;
    const int k = *slot = (int)(t.desc_next++ % bv_engine::TileJob::kDescRing);
    if (!t.h_desc[k]) {
        BV_HIP(e, hipHostMalloc(&t.h_desc[k], kDescBytes));
        BV_HIP(e, hipMalloc(&t.d_desc[k], kDescBytes));
        BV_HIP(e, hipEventCreateWithFlags(&t.ev_desc[k], hipEventDisableTiming));
    }
    if (t.desc_used[k]) BV_HIP(e, hipEventSynchronize(t.ev_desc[k]));  // the copy that last read this pinned table
    *h = t.h_desc[k];
    *d = t.d_desc[k];
    return BV_OK;
}
int desc_send(bv_engine *e, int slot, size_t bytes, hipStream_t st) {
    bv_engine::TileJob &t = e->tile;
    BV_HIP(e, hipMemcpyAsync(t.d_desc[slot], t.h_desc[slot], bytes, hipMemcpyHostToDevice, st));
    BV_HIP(e, hipEventRecord(t.ev_desc[slot], st));
    t.desc_used[slot] = true;
    return BV_OK;
}

// ---- the joined planes
uint8_t *joined_mq(bv_engine *e) { return e->tile.job.ranks ? e->tile.rows + e->tile.job.o_mq : nullptr; }
uint16_t *joined_rp(bv_engine *e) { return e->tile.job.ranks ? reinterpret_cast<uint16_t *>(e->tile.rows + e->tile.job.o_rp) : nullptr; }

// Before the job's first packed tile scatters into the joined planes: every column that has not been delivered yet says "nobody
// covered" (once per job; dense tiles that follow overwrite theirs)
int fill_uncovered_once(bv_engine *e, uint32_t tag, hipStream_t st) {
    Job &j = e->tile.job;
    if (j.filled) return BV_OK;
    uint8_t *jb = e->tile.rows, *jq = jb + j.o_q, *jm = joined_mq(e);
    uint16_t *jr = joined_rp(e);
    if (j.samples_seen == 0) {
        bv_launch_tile_fill_uncovered(jb, jq, jm, jr, (uint64_t)j.sites * j.pitch, tag, st);
        BV_HIP(e, hipGetLastError());
    } else {
        const size_t lo = j.samples_seen, w = j.samples_total - lo, S = j.sites;
        BV_HIP(e, hipMemset2DAsync(jb + lo, j.pitch, 0x08, w, S, st));
        BV_HIP(e, hipMemset2DAsync(jq + lo, j.pitch, 0, w, S, st));
        if (j.ranks) {
            BV_HIP(e, hipMemset2DAsync(jm + lo, j.pitch, 0, w, S, st));
            BV_HIP(e, hipMemset2DAsync(reinterpret_cast<uint8_t *>(jr) + 2 * lo, 2 * j.pitch, tag ? 0x80 : 0, 2 * w, S, st));
        }
    }
    j.filled = true;
    return BV_OK;
}

// ---- a packed tile's seven arrays
// ... as host planes to stage, in the order of bv_sparse_tile_packed_layout (rank planes / group ids only if the job has them)
void sparse_host_planes(const bv_sparse_tile &t, bool ranks, bool groups, HostPlane pl[7]) {
    const size_t E = t.n_entries;
    const HostPlane all[7] = {{t.row_start, 4 * ((size_t)t.n_sites + 1), nullptr}, {t.sample, 2 * E, nullptr}, {t.base_strand, E, nullptr}, {t.qual, E, nullptr},
                              {t.mapq, ranks && t.mapq ? E : 0, nullptr}, {t.rpr, ranks && t.rpr ? 2 * E : 0, nullptr},
                              {t.group_id, groups && t.group_id ? (size_t)t.n_samples : 0, nullptr}};
    std::copy(all, all + 7, pl);
}
// ... as the kernels get them (D: BvSparseTileArgs or BvSparseTileDesc): where `pl` was staged, or (NULL) the device tile's own
template <class D>
void sparse_device_arrays(D &d, const bv_sparse_tile &t, bool ranks, bool groups, const HostPlane *pl) {
    if (pl) {
        d.row_start = reinterpret_cast<const uint32_t *>(pl[0].dev); d.sample = reinterpret_cast<const uint16_t *>(pl[1].dev);
        d.call = pl[2].dev; d.phred = pl[3].dev; d.mapq = pl[4].dev; d.rank = reinterpret_cast<const uint16_t *>(pl[5].dev);
        d.group_id = pl[6].dev;
    } else {
        d.row_start = t.row_start; d.sample = t.sample; d.call = t.base_strand; d.phred = t.qual;
        d.mapq = ranks ? t.mapq : nullptr; d.rank = ranks ? t.rpr : nullptr; d.group_id = groups ? t.group_id : nullptr;
    }
    if (!t.n_entries) d.mapq = nullptr;  // (an empty tile reads no arrays but row_start)
}
// the job-wide fields of the packed-tile kernels' arguments
void sparse_job_args(bv_engine *e, BvSparseTileArgs &a) {
    const bv_engine::TileJob &t = e->tile;
    const Job &j = t.job;
    a.n_sites = j.sites;
    a.rpr_tag = rpr_tag(j);
    if (j.join) {
        a.bs = t.rows; a.q = t.rows + j.o_q; a.mq = joined_mq(e); a.rp = joined_rp(e); a.pitch = j.pitch;
    } else {
        a.n_groups = j.groups; a.stride = j.stride; a.rank_win = j.rank_win; a.hg_off = j.hg_off;
        a.ord_off = j.ord_off; a.ovf_cap = bv_engine::TileJob::kOvfCap; a.state = t.state; a.maxr = t.maxr; a.ovf = t.ovf;
    }
}

// ---- one checked tile, on a stream that job_stream has ordered
int add_dense_one(bv_engine *e, const bv_slab &t, hipStream_t st) {
    bv_engine::TileJob &tj = e->tile;
    Job &j = tj.job;
    j.layout = t.layout; j.layout_set = true;
    const uint8_t *bs = t.base_strand, *q = t.qual, *mq = j.ranks ? t.mapq : nullptr, *gid = j.groups ? t.group_id : nullptr;
    const uint16_t *rp = j.ranks ? t.rpr : nullptr;
    const size_t S = t.n_sites, P = t.pitch;
    StageSlot *slot = nullptr;
    if (t.mem_kind == BV_MEM_HOST) {
        HostPlane pl[5] = {{bs, S * P, nullptr}, {q, S * P, nullptr}, {mq, mq ? S * P : 0, nullptr},
                           {rp, rp ? S * P * 2 : 0, nullptr}, {gid, gid ? (size_t)t.n_samples : 0, nullptr}};
        int rc = stage_host_planes(e, pl, 5, 0, &slot, nullptr, st);
        if (rc != BV_OK) return rc;
        rc = stage_publish(e, slot, st);
        if (rc != BV_OK) return rc;
        bs = pl[0].dev; q = pl[1].dev; mq = pl[2].dev;
        rp = reinterpret_cast<const uint16_t *>(pl[3].dev);
        gid = pl[4].dev;
    }
    if (j.join) {
        const uint64_t lo = j.samples_seen, JP = j.pitch;
        const uint32_t w = t.n_samples, rows = t.n_sites;
        BvTileScatterArgs sc;
        sc.max_rows = rows;
        sc.n_planes = 0;
        auto plane = [&](uint8_t *dst, const uint8_t *src, uint64_t scale, uint32_t n_rows) {
            BvTileScatterPlane &p = sc.plane[sc.n_planes++];
            p.dst = dst; p.src = src; p.dst_pitch = scale * JP; p.src_pitch = scale * P; p.col_off = scale * lo;
            p.width_bytes = (uint32_t)(scale * w); p.n_rows = n_rows;
        };
        plane(tj.rows, bs, 1, rows);
        plane(tj.rows + j.o_q, q, 1, rows);
        if (mq) plane(tj.rows + j.o_mq, mq, 1, rows);
        if (rp) plane(tj.rows + j.o_rp, reinterpret_cast<const uint8_t *>(rp), 2, rows);
        if (gid) plane(tj.rows + j.o_gid, gid, 1, 1);  // one row: the tile's group ids, in the same launch
        bv_launch_tile_scatter(sc, st);
    } else {
        BvTileArgs a;
        a.bs = bs; a.q = q; a.mapq = mq; a.rpr = rp; a.group_id = gid; a.pitch = P; a.n_sites = t.n_sites;
        a.width = t.n_samples; a.n_groups = j.groups; a.stride = j.stride; a.state = tj.state;
        a.rank_win = j.rank_win; a.hg_off = j.hg_off;
        a.maxr = tj.maxr;
        a.ord_off = j.ord_off; a.col0 = j.samples_seen; a.ovf = tj.ovf; a.ovf_cap = bv_engine::TileJob::kOvfCap;
        a.rpr_tag = rpr_tag(j);
        bv_launch_tile_tally(a, st);
    }
    BV_HIP(e, hipGetLastError());
    if (slot) {
        int rc = stage_release(e, slot, st);
        if (rc != BV_OK) return rc;
    }
    j.samples_seen += t.n_samples;
    return mark_done(e, st);
}

// A tile as its covered cells only (include/basevar_amd.h): scattered into the joined planes, which hold "uncovered" wherever no
// tile has delivered yet (filled once, when the job's first packed tile arrives), or added to the per-site tallies entry by entry.
int add_sparse_one(bv_engine *e, const bv_sparse_tile &t, hipStream_t st) {
    bv_engine::TileJob &tj = e->tile;
    Job &j = tj.job;
    j.layout = t.layout; j.layout_set = true;
    const bool ranks = j.ranks, groups = j.groups != 0;
    StageSlot *slot = nullptr;
    HostPlane pl[7];
    if (t.mem_kind == BV_MEM_HOST) {
        sparse_host_planes(t, ranks, groups, pl);
        int rc = stage_host_planes(e, pl, 7, 0, &slot, nullptr, st);
        if (rc != BV_OK) return rc;
        rc = stage_publish(e, slot, st);
        if (rc != BV_OK) return rc;
    }
    BvSparseTileArgs a{};
    sparse_job_args(e, a);
    sparse_device_arrays(a, t, ranks, groups, slot ? pl : nullptr);
    a.width = t.n_samples; a.n_entries = t.n_entries;
    a.col0 = j.samples_seen;
    if (j.join) {
        int rc = fill_uncovered_once(e, a.rpr_tag, st);
        if (rc != BV_OK) return rc;
        if (t.n_entries) {
            bv_launch_tile_sparse_scatter(a, st);
            BV_HIP(e, hipGetLastError());
        }
        if (a.group_id) BV_HIP(e, hipMemcpyAsync(tj.rows + j.o_gid + j.samples_seen, a.group_id, t.n_samples, hipMemcpyDeviceToDevice, st));
    } else if (t.n_entries) {
        bv_launch_tile_sparse_tally(a, st);
        BV_HIP(e, hipGetLastError());
    }
    if (slot) {
        int rc = stage_release(e, slot, st);
        if (rc != BV_OK) return rc;
    }
    j.samples_seen += t.n_samples;
    return mark_done(e, st);
}
}  // namespace

void bv_impl::tile_job_free(bv_engine::TileJob &t) {
    for (int i = 0; i < bv_engine::TileJob::kDescRing; ++i) {
        if (t.h_desc[i]) (void)hipHostFree(t.h_desc[i]);
        if (t.d_desc[i]) (void)hipFree(t.d_desc[i]);
        if (t.ev_desc[i]) (void)hipEventDestroy(t.ev_desc[i]);
    }
    if (t.state) (void)hipFree(t.state);
    if (t.maxr) (void)hipFree(t.maxr);
    if (t.ovf) (void)hipFree(t.ovf);
    if (t.rows) (void)hipFree(t.rows);
}

extern "C" {

int bv_engine_tiles_begin(bv_engine *e, uint32_t n_sites, uint32_t n_samples_total, uint32_t n_groups, int with_ranks) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_tiles_begin: null engine");
    if (n_sites == 0 || n_samples_total == 0) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_begin: empty job");
    if (n_sites > e->cfg.max_sites) return fail(e, BV_ERR_TOO_LARGE, "bv_engine_tiles_begin: n_sites exceeds cfg.max_sites");
    if (n_groups > BV_MAX_GROUPS) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_begin: n_groups exceeds BV_MAX_GROUPS");
    // The job's state is cleared ON THE ENGINE'S STREAM, ordered like a submit (use_stream / mark_done): a tile added on another
    // stream waits for it.  (Until round 6 these were hipMemset calls on the null stream, which nothing orders against the engine's
    // non-blocking stream: a tally kernel could meet the state of a fresh allocation -- once in the round-6 campaigns, 8,037
    // mismatching fields in one 4,096-site job, gone on the re-run.)
    hipStream_t st0 = nullptr;
    {
        int rc = job_stream(e, nullptr, &st0);
        if (rc != BV_OK) return rc;
    }
    bv_engine::TileJob &t = e->tile;
    Job &j = t.job;
    j = Job{};  // whatever an earlier job left, finished or abandoned (a begin that fails below leaves no job open)
    j.sites = n_sites; j.groups = n_groups; j.samples_total = n_samples_total; j.ranks = with_ranks != 0;
    if (!(e->cfg.flags & BV_FLAG_TILE_STATE)) {
        // joined rows: [n_sites][pitch] planes resident in HBM, if they fit next to what is already there
        const size_t pitch = up256(n_samples_total), plane = (size_t)n_sites * pitch;
        const size_t o_q = plane, o_mq = 2 * plane, o_rp = o_mq + (with_ranks ? plane : 0), o_gid = o_rp + (with_ranks ? 2 * plane : 0),
                     need = o_gid + pitch;
        bool ok = need <= t.rows_bytes;
        if (!ok) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need <= (free_b + t.rows_bytes) / 10 * 9) {
                const int rc = try_grow_device(e, &t.rows, &t.rows_bytes, need);
                if (rc != BV_OK) return rc;
                ok = t.rows != nullptr;
            }
        }
        if (ok) {
            j.pitch = pitch; j.o_q = o_q; j.o_mq = o_mq; j.o_rp = o_rp; j.o_gid = o_gid;
            // (tiles fill the columns from the left in the order they are added; what a job leaves unfilled is set to 'N' at
            // finish -- not the whole plane here: 8.6 GB of memset for 8 Ki sites x 1 M samples)
            BV_HIP(e, hipMemsetAsync(t.rows + o_gid, 0xFF, pitch, st0));   // no pop-group
            j.join = true;
            j.open = true;
            return mark_done(e, st0);
        }
    }
    if (n_groups > BV_GROUPS_PER_ROUND)
        return fail(e, BV_ERR_TOO_LARGE, "bv_engine_tiles_begin: more than 32 pop-groups need the joined-rows realisation (2 KiB of "
                                         "per-site state per group otherwise), and the joined planes of this job do not fit the device");
    // H1 2048 + Hm 1024 + Hr 4 x W + Hg 512/group (bv_tiles.hip); W = 1024 ranks, or what the caller announced
    j.rank_win = with_ranks > 1 ? (uint32_t)((with_ranks + 1023) / 1024 * 1024) : 1024u;
    j.hg_off = 3072u + 4u * j.rank_win; j.ord_off = j.hg_off + n_groups * 512u; j.stride = j.ord_off + (1u + n_groups) * BV_TS_ORD_WORDS;
    if (!t.ovf) BV_HIP(e, hipMalloc(&t.ovf, sizeof(uint32_t) * (2u + 2u * (size_t)bv_engine::TileJob::kOvfCap)));
    BV_HIP(e, hipMemsetAsync(t.ovf, 0, 2 * sizeof(uint32_t), st0));
    const size_t bytes = (size_t)n_sites * j.stride * sizeof(uint32_t), mbytes = (size_t)n_sites * sizeof(uint32_t);
    int rc = grow_device(e, &t.state, &t.state_bytes, bytes);
    if (rc == BV_OK) rc = grow_device(e, &t.maxr, &t.maxr_bytes, mbytes);
    if (rc != BV_OK) return rc;
    BV_HIP(e, hipMemsetAsync(t.state, 0, bytes, st0));
    BV_HIP(e, hipMemsetAsync(t.maxr, 0, mbytes, st0));
    j.open = true;
    return mark_done(e, st0);
}

int bv_tile_packed_layout(uint32_t n_sites, uint32_t width, int with_ranks, int with_groups, uint64_t *pitch,
                          uint64_t offsets[5], uint64_t *total_bytes) {
    if (!n_sites || !width || !pitch || !offsets || !total_bytes)
        return fail(nullptr, BV_ERR_INVALID_ARG, "bv_tile_packed_layout: bad argument");
    const uint64_t P = ((uint64_t)width + 15) / 16 * 16, plane = up256((uint64_t)n_sites * P);
    uint64_t at = 0;
    offsets[0] = at; at += plane;
    offsets[1] = at; at += plane;
    offsets[2] = with_ranks ? at : 0; at += with_ranks ? plane : 0;
    offsets[3] = with_ranks ? at : 0; at += with_ranks ? up256((uint64_t)n_sites * P * 2) : 0;
    offsets[4] = with_groups ? at : 0; at += with_groups ? up256(P) : 0;
    *pitch = P;
    *total_bytes = at;
    return BV_OK;
}

int bv_sparse_tile_packed_layout(uint32_t n_sites, uint32_t n_entries, uint32_t width, int with_ranks, int with_groups,
                                 uint64_t offsets[7], uint64_t *total_bytes) {
    if (!n_sites || !width || !offsets || !total_bytes) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_sparse_tile_packed_layout: bad argument");
    const uint64_t E = n_entries ? n_entries : 1u;
    uint64_t at = 0;
    offsets[0] = at; at += up256(4ull * ((uint64_t)n_sites + 1));
    offsets[1] = at; at += up256(2 * E);
    offsets[2] = at; at += up256(E);
    offsets[3] = at; at += up256(E);
    offsets[4] = with_ranks ? at : 0; at += with_ranks ? up256(E) : 0;
    offsets[5] = with_ranks ? at : 0; at += with_ranks ? up256(2 * E) : 0;
    offsets[6] = with_groups ? at : 0; at += with_groups ? up256(width) : 0;
    *total_bytes = at;
    return BV_OK;
}

int bv_engine_tiles_add(bv_engine *e, const bv_slab *t, void *stream_) {
    if (!e || !t) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_add: null argument");
    if (!e->tile.job.open) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_add: call bv_engine_tiles_begin first");
    if (const char *why = check_dense_tile(e, *t, e->tile.job.samples_seen, t->layout))
        return fail(e, BV_ERR_INVALID_ARG, std::string("bv_engine_tiles_add: ") + why);
    hipStream_t st = nullptr;
    const int rc = job_stream(e, stream_, &st);
    return rc != BV_OK ? rc : add_dense_one(e, *t, st);
}

int bv_engine_tiles_add_sparse(bv_engine *e, const bv_sparse_tile *t, void *stream_) {
    if (!e || !t) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_add_sparse: null argument");
    if (!e->tile.job.open) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_add_sparse: call bv_engine_tiles_begin first");
    if (const char *why = check_sparse_tile(e, *t, e->tile.job.samples_seen, t->layout))
        return fail(e, BV_ERR_INVALID_ARG, std::string("bv_engine_tiles_add_sparse: ") + (why == kSparseSitesDiffer ? "tile " : "") + why);
    hipStream_t st = nullptr;
    const int rc = job_stream(e, stream_, &st);
    return rc != BV_OK ? rc : add_sparse_one(e, *t, st);
}

// Many packed tiles per call (include/basevar_amd.h): the records of n_tiles calls of bv_engine_tiles_add_sparse, but the tiles go
// in GROUPS -- at most BV_TILE_MANY_MAX tiles and kSparseManyStage bytes of host tiles -- and a group costs one staging slot (one
// copy per host tile into it), one descriptor table and ONE launch, where a tile cost a slot, two events, two waits and a launch of
// its own (~48 us per 200-sample tile of a 16,384-site job, round 6).  64 MiB: ~33 such tiles (1.9 MB each) per group, so the
// copies of the next group still run under the kernel of this one, and the four slots of the staging ring hold at most 256 MiB.
static constexpr size_t kSparseManyStage = (size_t)64 << 20;
int bv_engine_tiles_add_sparse_many(bv_engine *e, uint32_t n_tiles, const bv_sparse_tile *tiles, void *stream_) {
    if (!e || !tiles || n_tiles == 0) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_add_sparse_many: null / empty argument");
    Job &j = e->tile.job;
    if (!j.open) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_add_sparse_many: call bv_engine_tiles_begin first");
    // every tile is checked before anything changes: a refused call leaves the job as it was
    uint64_t seen = j.samples_seen;
    for (uint32_t k = 0; k < n_tiles; ++k) {
        if (const char *why = check_sparse_tile(e, tiles[k], seen, tiles[0].layout))
            return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_add_sparse_many: tile " + std::to_string(k) + ": " + why);
        seen += tiles[k].n_samples;
    }
    j.layout = tiles[0].layout; j.layout_set = true;
    hipStream_t st = nullptr;
    {
        int rc = job_stream(e, stream_, &st);
        if (rc != BV_OK) return rc;
    }
    const bool ranks = j.ranks, groups = j.groups != 0;
    BvSparseTileArgs a{};
    sparse_job_args(e, a);
    if (j.join) {
        int rc = fill_uncovered_once(e, a.rpr_tag, st);
        if (rc != BV_OK) return rc;
    }
    uint8_t *jgid = j.join && groups ? e->tile.rows + j.o_gid : nullptr;
    struct Staged {
        HostPlane pl[7];
        HostPlanes h;
    };
    std::vector<Staged> plan(n_tiles < (uint32_t)BV_TILE_MANY_MAX ? n_tiles : (uint32_t)BV_TILE_MANY_MAX);
    for (uint32_t k0 = 0, k1 = 0; k0 < n_tiles; k0 = k1) {
        // the group [k0, k1): its host tiles' staging bytes
        size_t bytes = 0;
        for (k1 = k0; k1 < n_tiles && k1 - k0 < (uint32_t)BV_TILE_MANY_MAX; ++k1) {
            Staged &p = plan[k1 - k0];
            p.h = HostPlanes{};
            if (tiles[k1].mem_kind == BV_MEM_HOST) {
                sparse_host_planes(tiles[k1], ranks, groups, p.pl);
                p.h = plan_host_planes(p.pl, 7);
            }
            if (k1 > k0 && bytes + p.h.bytes > kSparseManyStage) break;  // (a group holds at least one tile, however large)
            bytes += p.h.bytes;
        }
        const uint32_t nk = k1 - k0;
        StageSlot *slot = nullptr;
        if (bytes) {
            int rc = stage_acquire(e, bytes, &slot);
            if (rc != BV_OK) return rc;
            rc = stage_order(e, slot, st);
            if (rc != BV_OK) return rc;
            uint8_t *base = static_cast<uint8_t *>(slot->buf);
            size_t off = 0;
            for (uint32_t i = 0; i < nk; ++i) {
                Staged &p = plan[i];
                if (!p.h.bytes) continue;
                rc = copy_host_planes(e, p.pl, 7, p.h, base + off, slot->cs);
                if (rc != BV_OK) return rc;
                off += up256(p.h.bytes);
            }
        }
        // the descriptor table: pinned, then one copy on `st` (ahead of the wait for the staging copies)
        int ds = 0;
        void *h_tab = nullptr, *d_tab = nullptr;
        int rc = desc_acquire(e, &ds, &h_tab, &d_tab);
        if (rc != BV_OK) return rc;
        BvSparseTileDesc *tab = static_cast<BvSparseTileDesc *>(h_tab);
        uint64_t col = j.samples_seen;
        for (uint32_t i = 0; i < nk; ++i) {
            const bv_sparse_tile &t = tiles[k0 + i];
            sparse_device_arrays(tab[i], t, ranks, groups, plan[i].h.bytes ? plan[i].pl : nullptr);
            tab[i].col0 = col; tab[i].width = t.n_samples; tab[i].n_entries = t.n_entries;
            col += t.n_samples;
        }
        rc = desc_send(e, ds, sizeof(BvSparseTileDesc) * nk, st);
        if (rc == BV_OK && slot) rc = stage_publish(e, slot, st);
        if (rc != BV_OK) return rc;
        const BvSparseTileDesc *dtab = static_cast<const BvSparseTileDesc *>(d_tab);
        if (j.join) bv_launch_tile_sparse_scatter_many(a, dtab, nk, jgid, st);
        else bv_launch_tile_sparse_tally_many(a, dtab, nk, st);
        BV_HIP(e, hipGetLastError());
        if (slot) {
            rc = stage_release(e, slot, st);
            if (rc != BV_OK) return rc;
        }
        j.samples_seen = (uint32_t)col;
    }
    return mark_done(e, st);
}

// Several tiles at once.  Device-resident tiles of a joined-rows job go to their columns in ONE launch per <= 256 tiles
// (descriptor table in device memory); anything else -- host tiles, the per-site-tally realisation -- is added tile by tile.
int bv_engine_tiles_add_many(bv_engine *e, uint32_t n_tiles, const bv_slab *tiles, void *stream_) {
    if (!e || !tiles || n_tiles == 0) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_add_many: null / empty argument");
    bv_engine::TileJob &tj = e->tile;
    Job &j = tj.job;
    if (!j.open) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_add_many: call bv_engine_tiles_begin first");
    bool one_launch = j.join;
    uint64_t seen = j.samples_seen;
    for (uint32_t k = 0; k < n_tiles; ++k) {  // every tile is checked before anything is queued
        if (const char *why = check_dense_tile(e, tiles[k], seen, tiles[0].layout))
            return fail(e, BV_ERR_INVALID_ARG, std::string("bv_engine_tiles_add_many: ") + why);
        seen += tiles[k].n_samples;
        one_launch = one_launch && tiles[k].mem_kind != BV_MEM_HOST;
    }
    hipStream_t st = nullptr;
    {
        int rc = job_stream(e, stream_, &st);
        if (rc != BV_OK) return rc;
    }
    if (!one_launch) {
        for (uint32_t k = 0; k < n_tiles; ++k) {
            int rc = add_dense_one(e, tiles[k], st);
            if (rc != BV_OK) return rc;
        }
        return BV_OK;
    }
    j.layout = tiles[0].layout; j.layout_set = true;
    const uint64_t JP = j.pitch;
    for (uint32_t k0 = 0; k0 < n_tiles; k0 += BV_TILE_MANY_MAX) {
        const uint32_t nk = n_tiles - k0 < (uint32_t)BV_TILE_MANY_MAX ? n_tiles - k0 : (uint32_t)BV_TILE_MANY_MAX;
        int slot = 0;
        void *h_tab = nullptr, *d_tab = nullptr;
        int rc = desc_acquire(e, &slot, &h_tab, &d_tab);
        if (rc != BV_OK) return rc;
        // the usual job -- tiles of one width and pitch, every byte quantity a multiple of 8: whole destination rows are
        // gathered across the tiles (bv_tile_join_rows_kernel); anything else: one descriptor per tile and plane
        const bv_slab &t0 = tiles[k0];
        bool uniform = !((t0.n_samples | t0.pitch | j.samples_seen | JP) & 7u);
        for (uint32_t i = 0; i < nk && uniform; ++i) {
            const bv_slab &t = tiles[k0 + i];
            uniform = t.n_samples == t0.n_samples && t.pitch == t0.pitch &&
                      !(((uintptr_t)t.base_strand | (uintptr_t)t.qual | (uintptr_t)t.mapq | (uintptr_t)t.rpr | (uintptr_t)t.group_id) & 7u);
        }
        if (uniform) {
            const uint8_t **tab = static_cast<const uint8_t **>(h_tab);  // [5][nk] pointers
            for (uint32_t i = 0; i < nk; ++i) {
                const bv_slab &t = tiles[k0 + i];
                tab[0 * nk + i] = t.base_strand; tab[1 * nk + i] = t.qual; tab[2 * nk + i] = t.mapq;
                tab[3 * nk + i] = reinterpret_cast<const uint8_t *>(t.rpr); tab[4 * nk + i] = t.group_id;
            }
            rc = desc_send(e, slot, sizeof(void *) * 5 * nk, st);
            if (rc != BV_OK) return rc;
            const uint8_t *const *dtab = static_cast<const uint8_t *const *>(d_tab);
            const uint64_t lo = j.samples_seen;
            auto join = [&](uint8_t *dst, int k, uint64_t scale, uint32_t n_rows) {
                BvTileJoinArgs ja;
                ja.dst = dst; ja.srcs = dtab + (size_t)k * nk; ja.dst_pitch = scale * JP; ja.src_pitch = scale * t0.pitch; ja.col_off = scale * lo;
                ja.width_bytes = (uint32_t)(scale * t0.n_samples); ja.n_tiles = nk; ja.n_rows = n_rows;
                bv_launch_tile_join_rows(ja, st);
            };
            join(tj.rows, 0, 1, t0.n_sites);
            join(tj.rows + j.o_q, 1, 1, t0.n_sites);
            if (j.ranks) {
                join(tj.rows + j.o_mq, 2, 1, t0.n_sites);
                join(tj.rows + j.o_rp, 3, 2, t0.n_sites);
            }
            if (j.groups) join(tj.rows + j.o_gid, 4, 1, 1);
            BV_HIP(e, hipGetLastError());
            j.samples_seen += (uint64_t)nk * t0.n_samples;
            continue;
        }
        BvTileScatterPlane wide[5 * BV_TILE_MANY_MAX], narrow[5 * BV_TILE_MANY_MAX];
        uint32_t nw = 0, nn = 0;
        uint64_t uw = 0, un = 0;
        for (uint32_t i = 0; i < nk; ++i) {
            const bv_slab &t = tiles[k0 + i];
            const uint64_t lo = j.samples_seen, P = t.pitch;
            auto plane = [&](uint8_t *dst, const void *src, uint64_t scale, uint32_t n_rows) {
                BvTileScatterPlane p;
                p.dst = dst; p.src = static_cast<const uint8_t *>(src); p.dst_pitch = scale * JP; p.src_pitch = scale * P; p.col_off = scale * lo;
                p.width_bytes = (uint32_t)(scale * t.n_samples); p.n_rows = n_rows;
                const bool w8 = !((p.dst_pitch | p.col_off | p.src_pitch | p.width_bytes | (uint64_t)(uintptr_t)p.dst | (uint64_t)(uintptr_t)p.src) & 7u);
                if (w8) { wide[nw++] = p; const uint64_t u = (uint64_t)(p.width_bytes / 8u) * n_rows; if (u > uw) uw = u; }
                else { narrow[nn++] = p; const uint64_t u = (uint64_t)p.width_bytes * n_rows; if (u > un) un = u; }
            };
            plane(tj.rows, t.base_strand, 1, t.n_sites);
            plane(tj.rows + j.o_q, t.qual, 1, t.n_sites);
            if (j.ranks) {
                plane(tj.rows + j.o_mq, t.mapq, 1, t.n_sites);
                plane(tj.rows + j.o_rp, t.rpr, 2, t.n_sites);
            }
            if (j.groups) plane(tj.rows + j.o_gid, t.group_id, 1, 1);
            j.samples_seen += t.n_samples;
        }
        BvTileScatterPlane *tab = static_cast<BvTileScatterPlane *>(h_tab);
        std::memcpy(tab, wide, sizeof(BvTileScatterPlane) * nw);
        std::memcpy(tab + nw, narrow, sizeof(BvTileScatterPlane) * nn);
        rc = desc_send(e, slot, sizeof(BvTileScatterPlane) * (nw + nn), st);
        if (rc != BV_OK) return rc;
        bv_launch_tile_scatter_many(static_cast<const BvTileScatterPlane *>(d_tab), nw, nn, uw, un, st);
        BV_HIP(e, hipGetLastError());
    }
    return mark_done(e, st);
}

int bv_engine_tiles_finish(bv_engine *e, const uint8_t *ref_base, bv_site_result *out, bv_group_result *gout,
                           uint32_t mem_kind, void *stream_) {
    if (!e || !ref_base || !out) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_finish: null argument");
    bv_engine::TileJob &tj = e->tile;
    Job &j = tj.job;
    if (!j.open) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_finish: no open tile job");
    if (j.groups && !gout) return fail(e, BV_ERR_INVALID_ARG, "bv_engine_tiles_finish: job has groups, gout is NULL");
    hipStream_t st = nullptr;
    {
        int rc = job_stream(e, stream_, &st);
        if (rc != BV_OK) return rc;
    }
    const size_t S = j.sites, G = j.groups;
    const uint8_t *dref = ref_base;
    bv_site_result *dout = out;
    bv_group_result *dgout = gout;
    e->host_out = nullptr; e->host_gout = nullptr;
    StageSlot *slot = nullptr;
    if (mem_kind == BV_MEM_HOST) {
        HostPlane pl[1] = {{ref_base, S, nullptr}};
        const int rc = stage_records(e, pl, 1, S, G, out, gout, &slot, &dout, &dgout, st);
        if (rc != BV_OK) return rc;
        dref = pl[0].dev;
    }
    if (j.join) {
        j.open = false;
        if (j.samples_seen < j.samples_total && !j.filled)  // samples announced but never delivered: uncovered cells
        {
            BV_HIP(e, hipMemset2DAsync(tj.rows + j.samples_seen, j.pitch, 0x08, j.samples_total - j.samples_seen, S, st));
            // (tagged ranks: the same cells' rank words must say "no call" too -- 0x8080: the tag's bit 15, rank 128)
            if (j.ranks && rpr_tag(j))
                BV_HIP(e, hipMemset2DAsync(tj.rows + j.o_rp + 2 * (size_t)j.samples_seen, 2 * j.pitch, 0x80,
                                           2 * (size_t)(j.samples_total - j.samples_seen), S, st));
        }
        RowLaunch L;
        L.bs = tj.rows; L.q = tj.rows + j.o_q; L.mq = joined_mq(e); L.rp = joined_rp(e); L.refb = dref; L.gid = G ? tj.rows + j.o_gid : nullptr;
        L.pitch = j.pitch; L.n_sites = j.sites; L.n_samples = j.samples_total; L.n_groups = j.groups; L.layout = j.layout;
        L.dout = dout; L.dgout = dgout;
        int rc = launch_passes(e, L, st);
        if (rc == BV_OK && slot) rc = stage_release(e, slot, st);
        return rc;
    }
    BV_HIP(e, hipMemsetAsync(e->d_counters, 0, sizeof(uint32_t) * BV_CTR_PER_LAUNCH * BV_CTR_STRIDE, st));
    if (G) BV_HIP(e, hipMemsetAsync(dgout, 0, S * G * sizeof(bv_group_result), st));
    BvTileFinishArgs f;
    f.state = tj.state; f.maxr = tj.maxr; f.ref_base = dref; f.n_sites = j.sites; f.n_groups = j.groups;
    f.stride = j.stride; f.have_ranks = j.ranks ? 1u : 0u; f.min_af = e->cfg.min_af; f.tables = e->d_tables;
    f.rank_win = j.rank_win; f.hg_off = j.hg_off;
    f.ord_off = j.ord_off; f.ovf = tj.ovf; f.ovf_cap = bv_engine::TileJob::kOvfCap;
    f.out = dout; f.gout = dgout; f.var_list = e->d_var_list; f.counters = e->d_counters;
    bv_launch_tile_finish(f, st);
    BV_HIP(e, hipGetLastError());
    e->last_ctr_base = 0; e->ctr_rot = 0;
    BV_HIP(e, hipMemcpyAsync(e->h_counters, e->d_counters, sizeof(uint32_t) * BV_CTR_WORDS * bv_engine::kCtrBlocks, hipMemcpyDeviceToHost, st));
    int rc = copy_records_back(e, st);
    if (rc != BV_OK) return rc;
    j.open = false;
    e->submitted = true;
    e->last_slot = -1;  // no pass-1/pass-2 event triplet for this realisation: bv_engine_kernel_ms has nothing to report
    if (slot) {
        rc = stage_release(e, slot, st);
        if (rc != BV_OK) return rc;
    }
    return mark_done(e, st);
}

}  // extern "C"
