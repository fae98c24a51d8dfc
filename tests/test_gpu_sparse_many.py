"""GPU tests (-m gpu) of bv_engine_tiles_add_sparse_many: many packed tiles (their covered cells only, include/basevar_amd.h) per
call.  The bar is the one of the call it batches: the records of n_tiles calls of bv_engine_tiles_add_sparse, byte for byte, in
both realisations of the tile mode -- which test_gpu_tagged.py holds to the dense tiles and the dense tiles to the rows and the
reference -- through the groups the engine cuts a call into, in jobs that mix every way of adding tiles, and all or nothing
when a tile of the call is refused."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from basevar_amd.synth import make_slab, tag_ranks
from test_gpu_parity import bv, check, oracle_run, run_engine  # noqa: F401  (bv: the module fixture)

ALL = 1 << 30  # sparse_batch: every packed tile of the job in one call


def same(a, b):
    assert a.sites.tobytes() == b.sites.tobytes(), [f for f in a.sites.dtype.names if not np.array_equal(a.sites[f], b.sites[f], equal_nan=a.sites[f].dtype.kind == "f")]
    if a.groups is not None or b.groups is not None:
        assert a.groups.tobytes() == b.groups.tobytes()
    assert a.n_variant == b.n_variant


def tiles_job(bv, slab, width, flags=0, **kw):
    eng = bv.BaseTypeEngine(max_sites=slab["base_strand"].shape[0], min_af_value=bv.min_af(int(slab.get("n_samples", slab["base_strand"].shape[1]))),
                            device=0, flags=flags)
    try:
        return eng.lrt_tiles(slab, width, **kw)
    finally:
        eng.close()


# ---- tiles built by hand (the error paths, device-resident tiles, several ways of adding tiles in one job)
def sparse_tile(slab, lo, w, one_allocation=True, device=False, layout=0):
    """columns [lo, lo + w) of a slab as a packed tile: (bv_sparse_tile, what must stay alive).  one_allocation: the layout of
    bv_sparse_tile_packed_layout (one copy over the link), else one numpy array per field; device: torch tensors on cuda:0."""
    from basevar_amd import _capi
    S = slab["base_strand"].shape[0]
    ranks = "mapq" in slab and "rpr" in slab
    ng = int(slab.get("n_groups", 0)) if slab.get("group_id") is not None else 0
    cb = slab["base_strand"][:, lo:lo + w]
    rows, cols = np.nonzero(cb != 8)
    E = int(rows.size)
    rs = np.zeros(S + 1, dtype=np.uint32)
    rs[1:] = np.cumsum(np.bincount(rows, minlength=S))
    fields = [rs, cols.astype(np.uint16), cb[rows, cols].astype(np.uint8), slab["qual"][:, lo:lo + w][rows, cols].astype(np.uint8)]
    if ranks:
        fields += [slab["mapq"][:, lo:lo + w][rows, cols].astype(np.uint8), (slab["rpr"][:, lo:lo + w][rows, cols] & 0x1FFF).astype(np.uint16)]
    else:
        fields += [None, None]
    fields.append(np.ascontiguousarray(slab["group_id"][lo:lo + w], dtype=np.uint8) if ng else None)
    keep = []
    if device:
        import torch
        ptrs = []
        for a in fields:
            if a is None:
                ptrs.append(None)
                continue
            t = torch.from_numpy(a.view(np.uint8).copy() if a.size else np.zeros(16, dtype=np.uint8)).to("cuda:0")
            keep.append(t)
            ptrs.append(t.data_ptr())
        kind = _capi.BV_MEM_DEVICE
    elif one_allocation:
        offs = (C.c_uint64 * 7)()
        total = C.c_uint64()
        assert _capi.load().bv_sparse_tile_packed_layout(S, E, w, 1 if ranks else 0, 1 if ng else 0, offs, C.byref(total)) == 0
        buf = np.zeros(total.value + 256, dtype=np.uint8)
        pad = (-buf.ctypes.data) % 256
        ptrs = []
        for k, a in enumerate(fields):
            if a is None:
                ptrs.append(None)
                continue
            raw = a.view(np.uint8)
            buf[pad + offs[k]: pad + offs[k] + raw.size] = raw
            ptrs.append(buf.ctypes.data + pad + offs[k])
        keep.append(buf)
        kind = _capi.BV_MEM_HOST
    else:
        fields = [None if a is None else np.ascontiguousarray(a) for a in fields]
        keep.extend(fields)
        ptrs = [None if a is None or a.size == 0 else a.ctypes.data for a in fields]
        ptrs[0] = fields[0].ctypes.data
        kind = _capi.BV_MEM_HOST
    return _capi.SparseTile(S, w, E, ng, *ptrs, kind, layout), keep


def dense_tile(slab, lo, w, layout=0):
    """columns [lo, lo + w) as a dense host tile (bv_slab, planes one numpy array each)"""
    from basevar_amd import _capi
    S = slab["base_strand"].shape[0]
    P = (w + 15) // 16 * 16
    planes = []
    for k, dt, fill in (("base_strand", np.uint8, 8), ("qual", np.uint8, 0), ("mapq", np.uint8, 0), ("rpr", np.uint16, 0)):
        a = np.full((S, P), fill, dtype=dt)
        a[:, :w] = slab[k][:, lo:lo + w]
        planes.append(a)
    ng = int(slab.get("n_groups", 0)) if slab.get("group_id") is not None else 0
    g = None
    if ng:
        g = np.full(P, 0xFF, dtype=np.uint8)
        g[:w] = slab["group_id"][lo:lo + w]
        planes.append(g)
    t = _capi.Slab(S, w, P, planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, planes[3].ctypes.data, None,
                   g.ctypes.data if ng else None, ng, _capi.BV_MEM_HOST, layout)
    return t, planes


def finish(eng, slab):
    from basevar_amd import _capi
    S = slab["base_strand"].shape[0]
    ng = int(slab.get("n_groups", 0)) if slab.get("group_id") is not None else 0
    ref = np.ascontiguousarray(slab["ref_base"], dtype=np.uint8)
    out = np.zeros(S, dtype=_capi.SITE_DTYPE)
    gout = np.zeros((S, ng), dtype=_capi.GROUP_DTYPE) if ng else None
    assert eng._lib.bv_engine_tiles_finish(eng._h, ref.ctypes.data, out.ctypes.data, gout.ctypes.data if ng else None, _capi.BV_MEM_HOST, None) == 0, eng._err()
    eng.wait()
    from basevar_amd.engine import BaseTypeBatch
    return BaseTypeBatch(out, gout, eng.last_variant_count(), 0.0, 0.0)


def add_many(eng, tiles):
    from basevar_amd import _capi
    arr = (_capi.SparseTile * len(tiles))(*tiles)
    return eng._lib.bv_engine_tiles_add_sparse_many(eng._h, len(tiles), arr, None)


# ---- 1. the parity grid of test_packed_host_tiles_give_the_dense_tiles_records
@pytest.mark.parametrize("flags", [0, 0x8], ids=["joined_rows", "per_site_tallies"])
@pytest.mark.parametrize("n,width,groups,tagged", [(3001, 200, 0, False), (1000, 200, 2, True), (70000, 5000, 0, True), (10000, 1000, 3, False), (640, 64, 0, False)])
def test_batched_packed_tiles_give_the_per_tile_records(bv, n, width, groups, tagged, flags):
    """sparse_batch 1, 7 and all: the records of one bv_engine_tiles_add_sparse per tile, of the dense tiles and (joined rows) of
    the rows, byte for byte; and in a job that mixes dense and packed tiles (every third tile dense)."""
    slab = make_slab(60, n, seed=1900 + n % 13, coverage=0.1, n_groups=groups, ref_n_frac=0.02)
    slab["rpr"][7, np.nonzero(slab["base_strand"][7] < 8)[0][:5]] = 700
    if tagged:
        slab = tag_ranks(slab)
    per_tile = tiles_job(bv, slab, width, flags, packed=True)
    dense = tiles_job(bv, slab, width, flags)
    same(dense, per_tile)
    if flags == 0:
        same(run_engine(bv, slab, bv.min_af(n)), per_tile)
    for sb in (1, 7, ALL):
        same(per_tile, tiles_job(bv, slab, width, flags, packed=True, sparse_batch=sb))
    same(per_tile, tiles_job(bv, slab, width, flags, packed=3, sparse_batch=7))
    assert per_tile.n_variant >= 2


# ---- 2. calls the engine cuts into several groups
@pytest.mark.parametrize("flags", [0, 0x8], ids=["joined_rows", "per_site_tallies"])
def test_more_tiles_than_one_launch_takes(bv, flags):
    """600 tiles of 16 samples in one call: more than BV_TILE_MANY_MAX (256) descriptors -> three groups."""
    slab = make_slab(40, 9600, seed=77, coverage=0.15, n_groups=2)
    per_tile = tiles_job(bv, slab, 16, flags, packed=True)
    same(per_tile, tiles_job(bv, slab, 16, flags, packed=True, sparse_batch=ALL))
    same(per_tile, tiles_job(bv, slab, 16, flags, packed=True, sparse_batch=300))
    if flags == 0:
        same(run_engine(bv, slab, bv.min_af(9600)), per_tile)


@pytest.mark.parametrize("flags", [0, 0x8], ids=["joined_rows", "per_site_tallies"])
def test_more_host_bytes_than_one_staging_slot_takes(bv, flags):
    """Wide, deep tiles: one of ~70 MB (beyond the 64 MiB a group stages: a group of its own), then seven of ~12 MB (several
    per group), host tiles in one allocation and in separate arrays, in one call -- the records of one call per tile."""
    from basevar_amd import _capi
    rng = np.random.default_rng(5)
    S = 512
    widths = [65536] * 8
    cov = [0.3] + [0.05] * 7
    N = sum(widths)
    tiles, keep = [], []
    lo = 0
    ref = rng.integers(0, 4, S).astype(np.uint8)
    for k, (w, c) in enumerate(zip(widths, cov)):
        part = {"base_strand": np.where(rng.random((S, w), dtype=np.float32) < c, rng.integers(0, 8, (S, w), dtype=np.uint8), np.uint8(8)),
                "qual": rng.integers(2, 42, (S, w), dtype=np.uint8), "mapq": rng.integers(0, 61, (S, w), dtype=np.uint8),
                "rpr": rng.integers(1, 151, (S, w), dtype=np.uint16)}
        t, kp = sparse_tile(part, 0, w, one_allocation=(k % 2 == 0))
        tiles.append(t)
        keep.append(kp)
        del part
        lo += w
    assert tiles[0].n_entries * 7 > (64 << 20) and all(t.n_entries * 7 < (16 << 20) for t in tiles[1:])
    recs = []
    maf = bv.min_af(N)
    for batched in (False, True):
        eng = bv.BaseTypeEngine(max_sites=S, min_af_value=maf, device=0, flags=flags)
        assert eng._lib.bv_engine_tiles_begin(eng._h, S, N, 0, 1) == 0, eng._err()
        if batched:
            assert add_many(eng, tiles) == 0, eng._err()
        else:
            for t in tiles:
                assert eng._lib.bv_engine_tiles_add_sparse(eng._h, C.byref(t), None) == 0, eng._err()
        recs.append(finish(eng, {"base_strand": np.zeros((S, 1), np.uint8), "ref_base": ref}))
        eng.close()
    same(recs[0], recs[1])
    assert (recs[0].sites["total_depth"] > 0).all() and recs[0].n_variant > 0


# ---- 3. one job, every way of adding tiles
@pytest.mark.parametrize("flags", [0, 0x8], ids=["joined_rows", "per_site_tallies"])
@pytest.mark.parametrize("groups", [0, 2])
def test_one_job_mixes_every_way_of_adding_tiles(bv, flags, groups):
    """tiles_add, tiles_add_many, tiles_add_sparse and tiles_add_sparse_many interleaved in one job; device-resident packed tiles
    (torch) beside host tiles (one allocation and separate arrays) in one call; empty tiles; a narrow last tile."""
    from basevar_amd import _capi
    S, n = 56, 3000 + 37
    slab = make_slab(S, n, seed=4242 + groups, coverage=0.12, n_groups=groups)
    slab["base_strand"][:, 1000:1100] = 8   # columns nobody covers: the tiles over them are empty packed tiles
    maf = bv.min_af(n)
    want = tiles_job(bv, slab, 100, flags)  # dense tiles of 100 samples
    if flags == 0:
        same(run_engine(bv, slab, maf), want)
    eng = bv.BaseTypeEngine(max_sites=S, min_af_value=maf, device=0, flags=flags)
    assert eng._lib.bv_engine_tiles_begin(eng._h, S, n, groups, 1) == 0, eng._err()
    keep = []

    def sp(lo, w, **kw):
        t, k = sparse_tile(slab, lo, w, **kw)
        keep.append(k)
        return t
    # [0, 300): dense, one call each
    for lo in (0, 100, 200):
        t, k = dense_tile(slab, lo, 100)
        keep.append(k)
        assert eng._lib.bv_engine_tiles_add(eng._h, C.byref(t), None) == 0, eng._err()
    # [300, 700): packed, one call with device, host and host-array tiles of different widths
    assert add_many(eng, [sp(300, 50, device=True), sp(350, 150), sp(500, 120, one_allocation=False), sp(620, 80, device=True)]) == 0, eng._err()
    # [700, 1000): dense, tiles_add_many
    d = [dense_tile(slab, lo, 100) for lo in (700, 800, 900)]
    keep.append(d)
    eng.tiles_add_many([t for t, _ in d])
    # [1000, 1100): two empty packed tiles (host and device) in a call with a covered one; then one add_sparse
    eng.tiles_add_sparse_many([sp(1000, 60), sp(1060, 40, device=True), sp(1100, 200)])
    assert eng._lib.bv_engine_tiles_add_sparse(eng._h, C.byref(sp(1300, 200)), None) == 0, eng._err()
    # [1500, n): packed tiles of 500 in one call, the last one narrow (37 samples)
    eng.tiles_add_sparse_many([sp(lo, min(500, n - lo), device=(lo // 500) % 2 == 1) for lo in range(1500, n, 500)])
    got = finish(eng, slab)
    eng.close()
    same(want, got)
    assert got.n_variant >= 2


# ---- 4. shallow sites whose cells come from several tiles of one call
def test_shallow_tied_sites_from_several_tiles_of_one_call(bv, restatement):
    """Per-site tallies: the cells of one launch reach a shallow site's ordered list in any order; finish() sorts them by sample
    index (bv_tile_sorted_cells), so the replay in the reference's per-sample order -- exact two- and three-way ties included --
    gives the row kernels' calls and the oracle's records, with no tie excused."""
    n, S = 900, 48
    slab = make_slab(S, n, seed=4100, coverage=0.01, n_groups=3, site_offset=1)
    rng = np.random.default_rng(4)
    for site in range(0, S, 3):   # exact ties, the cells far apart: in different tiles
        slab["base_strand"][site, :] = 8
        cols = np.sort(rng.permutation(n)[:3])
        k = 2 + (site // 3) % 2
        slab["base_strand"][site, cols[:k]] = [(slab["ref_base"][site] + 1 + j) % 4 for j in range(k)]
        slab["qual"][site, :] = 0
        slab["qual"][site, cols[:k]] = 30
        slab["mapq"][site, cols[:k]] = 60
        slab["rpr"][site, cols[:k]] = 10
    for site in range(1, S, 3):   # up to 64 covered cells spread over the whole row
        slab["base_strand"][site, :] = 8
        cols = rng.permutation(n)[:40 + site % 25]
        slab["base_strand"][site, cols] = rng.integers(0, 8, cols.size)
    maf = bv.min_af(n)
    eng = bv.BaseTypeEngine(max_sites=S, min_af_value=maf, device=0, flags=0x8)
    rows = eng.lrt(slab)
    eng.close()
    for width in (64, 7):
        per_tile = tiles_job(bv, slab, width, 0x8, packed=True)
        t = tiles_job(bv, slab, width, 0x8, packed=True, sparse_batch=ALL)
        same(per_tile, t)
        for f in ("n_alt", "alt", "depth", "total_depth", "af", "chi2"):
            assert np.array_equal(rows.sites[f], t.sites[f], equal_nan=True), (width, f)
    exp, gexp, margins = oracle_run(restatement, slab, maf)
    assert check(t, exp, gexp, margins) == 0


# ---- 5. BASELINE configs[4]'s row length
@pytest.mark.parametrize("flags", [0, 0x8], ids=["joined_rows", "per_site_tallies"])
def test_64_sites_x_one_million_samples_in_batches(bv, restatement, flags):
    """64 sites x 1,000,000 samples: 5000 packed host tiles of 200 samples in calls of 256, with two pop-groups, against the
    restatement (the real reference where oracle/_ref is present) and the rows."""
    import oracle
    n = 1000000
    parts = [make_slab(8, n, seed=600 + k, coverage=0.05, n_groups=2, site_offset=8 * k) for k in range(8)]
    slab = {k: np.concatenate([p[k] for p in parts]) for k in ("base_strand", "qual", "mapq", "rpr", "ref_base")}
    slab.update(n_sites=64, n_samples=n, pitch=parts[0]["pitch"], n_groups=2, group_id=parts[0]["group_id"])
    del parts
    maf = bv.min_af(n)
    eng = bv.BaseTypeEngine(max_sites=64, min_af_value=maf, device=0, flags=flags)
    t = eng.lrt_tiles(slab, 200, packed=True, sparse_batch=256)
    rows = eng.lrt(slab)
    eng.close()
    if oracle.ref_available():
        exp, gexp = oracle.Reference().run(slab, maf, n_threads=16)
        check(t, exp, gexp, check_chi2=False)
    else:
        exp, gexp, margins = restatement.run_with_margins(slab, maf, n_threads=16)
        check(t, exp, gexp, margins)
    assert ((exp["status"] & 2) != 0).sum() >= 8
    for f in ("depth", "total_depth", "cvg_sb", "var_sb", "n_alt", "alt"):
        assert np.array_equal(rows.sites[f], t.sites[f]), f
    if flags == 0:
        assert rows.sites.tobytes() == t.sites.tobytes() and rows.groups.tobytes() == t.groups.tobytes()


# ---- 6. refused calls change nothing
@pytest.mark.parametrize("flags", [0, 0x8], ids=["joined_rows", "per_site_tallies"])
def test_a_refused_call_leaves_the_job_as_it_was(bv, flags):
    from basevar_amd import _capi
    INV = _capi.BV_ERR_INVALID_ARG
    S, n, w = 40, 1200, 200
    slab = make_slab(S, n, seed=31, coverage=0.2, n_groups=2)
    maf = bv.min_af(n)
    want = tiles_job(bv, slab, w, flags)
    eng = bv.BaseTypeEngine(max_sites=S, min_af_value=maf, device=0, flags=flags)
    keep = []

    def sp(lo, ww=w, **kw):
        t, k = sparse_tile(slab, lo, ww, **kw)
        keep.append(k)
        return t
    good = [sp(lo) for lo in range(0, n, w)]
    # no open job; NULL / zero tiles
    assert add_many(eng, good[:2]) == INV
    assert eng._lib.bv_engine_tiles_begin(eng._h, S, n, 2, 1) == 0, eng._err()
    assert eng._lib.bv_engine_tiles_add_sparse_many(eng._h, 2, None, None) == INV
    assert eng._lib.bv_engine_tiles_add_sparse_many(eng._h, 0, (_capi.SparseTile * 1)(good[0]), None) == INV
    # every refusal comes AFTER good tiles in the same call, and after a tagged good tile (the job's layout must stay unset)
    tagged = sp(0, layout=_capi.BV_SLAB_RPR_TAGGED)

    def bad(**change):
        t, k = sparse_tile(slab, 200, w)
        keep.append(k)
        for f, v in change.items():
            setattr(t, f, v)
        return t
    wrong_sites = bad(n_sites=S - 1)
    rs_bad = []
    for how in ("start", "decrease", "end"):
        t, k = sparse_tile(slab, 200, w, one_allocation=False)
        keep.append(k)
        rs = np.ctypeslib.as_array(C.cast(t.row_start, C.POINTER(C.c_uint32)), shape=(S + 1,))
        if how == "start":
            rs[0] = 1
        elif how == "decrease":
            rs[5], rs[6] = rs[6] + 1, rs[6]
        else:
            rs[S] = rs[S] + 1
        rs_bad.append(t)
    cases = [[tagged, good[1], wrong_sites]] + [[good[0], t] for t in rs_bad] + [
        [tagged, good[1]],                                              # mismatched layouts inside one call
        [good[0], good[1], bad(layout=2)],                              # an unknown layout bit
        [good[0], bad(n_samples=70000)],                                # more than 65,536 samples in a tile
        [good[0], bad(row_start=None)],                                 # a missing array
        [good[0], bad(group_id=None)],                                  # the job has groups
        [good[0], bad(mapq=None)],                                      # the job has rank planes
        good + [good[0]],                                               # more samples than announced (the call's sum)
    ]
    for k, c in enumerate(cases):
        assert add_many(eng, c) == INV, k
    # ... and the job takes the good tiles and gives the records of the dense tiles
    assert add_many(eng, good[:2]) == 0, eng._err()
    assert add_many(eng, [good[0]] * 2 + good[2:]) == INV   # (still all or nothing after a good call)
    assert add_many(eng, good[2:]) == 0, eng._err()
    assert add_many(eng, good[:1]) == INV   # the job is full
    got = finish(eng, slab)
    eng.close()
    same(want, got)
