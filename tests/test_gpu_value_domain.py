"""GPU tests (-m gpu) over the whole value domain of the mapq, phred and rank planes (tests/value_domain.py): mapq 0..255,
phred 0..93 and ranks 0..65,535 on the REF and ALT reads of variant sites, through every kernel form a row length selects
(asserted with BaseTypeEngine.last_launch_form), the diagnostic flags, pop-groups from 3 to 40, both rank layouts, chained
submits, tile jobs in both realisations, and batchfile text rows.  Every record is held to the oracle with its margins, and
no site may be excused as a tie."""
import numpy as np
import pytest

import basevar_amd

pytestmark = pytest.mark.gpu

from basevar_amd.engine import BaseTypeBatch
from basevar_amd.synth import tag_ranks
from test_gpu_parity import bv, check, oracle_run  # noqa: F401  (bv: the module fixture)
from test_gpu_tagged import same
from test_gpu_text_rows import check as text_check
from value_domain import assert_edges_hit, dense_slab, edge_slab, ranksum_sites, read_classes

# BV_FORM_* and the diagnostic flags (include/basevar_amd_diag.h)
SHORT_ROWS, ONE_KERNEL, PASS2_FUSED = 0x1, 0x2, 0x4
WAVE_SOLVER, PASS2_SWEEP, NO_DOM, P2_TAIL_DMA = 0x10, 0x20, 0x1000000, 0x2000000
TILE_STATE = 0x8  # BV_FLAG_TILE_STATE: the per-site-tally realisation of tile jobs
RPR_RANGE = 0x40  # BV_SITE_RPR_RANGE


def short_row_form(k):
    return (k & 0xF) << 12


def long_row_form(k):
    return (k & 0xF) << 8


def expected_form(n, flags=0):
    """The BV_FORM_* bits a submit of rows of n samples (with rank planes) must report (csrc/bv_engine_rows.hip)."""
    if n > 49152:
        return ONE_KERNEL  # the long-row kernel
    form = (flags >> 12) & 0xF
    if form != 9 and (n + 15) // 16 > 256:  # three 4 KiB slots of the fused kernel: rows of 4,097 samples and more
        return SHORT_ROWS | ONE_KERNEL | (PASS2_FUSED if form != 10 and not flags & PASS2_SWEEP else 0)
    return SHORT_ROWS  # streaming + solve kernels, pass 2 a launch of its own


def coverage_for(n):
    return 0.5 if n <= 64 else 0.2 if n <= 4096 else 0.1 if n <= 16385 else 0.08


def sites_for(n):
    return 240 if n <= 64 else 160 if n <= 2048 else 128 if n <= 4096 else 64 if n <= 16385 else 40


def lrt(bv, slab, flags=0):
    """(records, BV_FORM_* bits) of one submit."""
    eng = bv.BaseTypeEngine(max_sites=slab["base_strand"].shape[0], min_af_value=bv.min_af(slab["n_samples"]), device=0, flags=flags)
    try:
        got = eng.lrt(slab)
        return got, eng.last_launch_form()
    finally:
        eng.close()


def exact(restatement, got, slab, exp=None):
    """got == the oracle's records of `slab` (plain ranks), no site excused as a tie.  Returns the oracle's (records, group
    records, margins) for reuse."""
    if exp is None:
        exp = oracle_run(restatement, slab, basevar_amd.min_af(slab["n_samples"]), n_threads=16)
    e, g, margins = exp
    assert check(got, e, g, margins) == 0, "a site needed the tie excuse"
    return exp


ROWS = [60, 1500, 2048, 2049, 4096, 4097, 16384, 16385, 49152, 49153, 70000]


@pytest.mark.parametrize("n", ROWS)
def test_row_lengths_reach_every_kernel_form(bv, restatement, n):
    """One row length per kernel form: <= 64 covered (the per-sample replay), three launches with workgroup-per-row pass 2
    (<= 2,048) and LDS-DMA pass 2 (<= 4,096), the fused kernel (<= 49,152), the long-row kernel.  Ranks up to 65,535 (plain
    layout), and a second slab with ranks up to 8,191 whose tagged layout must give the plain layout's records byte for byte."""
    for max_rank in (65535, 8191):
        slab = edge_slab(sites_for(n), n, seed=n + max_rank, coverage=coverage_for(n), max_rank=max_rank)
        got, form = lrt(bv, slab)
        assert form == expected_form(n), "form 0x%x" % form
        exact(restatement, got, slab)
        assert_edges_hit(slab, got, max_rank=max_rank)
        if max_rank <= 8191:
            tagged, tform = lrt(bv, tag_ranks(slab))
            assert tform == form
            same(got, tagged)


@pytest.mark.parametrize("flags,n,groups,identical", [
    # the fused kernel's rank-sum rows through its LDS-DMA rings, not registers
    pytest.param(P2_TAIL_DMA, 16384, 0, True, id="p2_tail_dma-16384"),
    pytest.param(P2_TAIL_DMA, 49152, 0, True, id="p2_tail_dma-49152"),
    # the fused kernel for pass 1, pass 2 a launch of its own; the three launches of shorter rows
    pytest.param(short_row_form(10), 16385, 0, True, id="short_row_form_10-16385"),
    pytest.param(short_row_form(9), 4097, 0, True, id="short_row_form_9-4097"),
    pytest.param(short_row_form(9), 49152, 0, True, id="short_row_form_9-49152"),
    # plain-load pass-2 kernels instead of the LDS-DMA one
    pytest.param(PASS2_SWEEP, 2049, 0, False, id="pass2_sweep-2049"),
    pytest.param(PASS2_SWEEP, 16384, 0, False, id="pass2_sweep-16384"),
    # the long-row kernel without the team helpers
    pytest.param(long_row_form(2), 49153, 0, True, id="long_row_form_2-49153"),
    pytest.param(long_row_form(2), 70000, 0, True, id="long_row_form_2-70000"),
    # every candidate and pop-group call on the one-per-wave solver
    pytest.param(WAVE_SOLVER, 1500, 3, False, id="wave_solver-1500-groups"),
    pytest.param(WAVE_SOLVER, 16384, 3, False, id="wave_solver-16384-groups"),
])
def test_diagnostic_flags(bv, restatement, flags, n, groups, identical):
    """Every flag meets the oracle; where the diag header says records do not depend on it, they equal the default path's
    byte for byte.  Both layouts (tagged on the slab whose ranks stop at 8,191)."""
    for max_rank in (65535, 8191):
        slab = edge_slab(sites_for(n), n, seed=7 * n + max_rank + flags % 977, coverage=coverage_for(n), n_groups=groups, max_rank=max_rank)
        exp = None
        for s in [slab] + ([tag_ranks(slab)] if max_rank <= 8191 else []):
            base, f0 = lrt(bv, s)
            got, f1 = lrt(bv, s, flags)
            assert f0 == expected_form(n) and f1 == expected_form(n, flags), "forms 0x%x 0x%x" % (f0, f1)
            exp = exact(restatement, got, slab, exp)
            exact(restatement, base, slab, exp)
            if identical:
                same(base, got)
        assert_edges_hit(slab, exp[0], max_rank=max_rank)


@pytest.mark.parametrize("n,sites", [(1500, 60), (3000, 60), (12000, 40), (70000, 10)])
def test_dense_rows_dominant_mapq(bv, restatement, n, sites):
    """Deep rows take the dominant-value count in the rank-sum mapq tally (bv_lds_add16_dom): dominant mapq 60, 0 and 255, a
    first passing lane whose value no other lane holds, REF and ALT reads with different dominant values.  Records: the
    oracle's, and byte-identical to those of the plain adds (BV_FLAG_NO_DOM), in both rank layouts."""
    slab = dense_slab(sites, n, seed=5000 + n)
    is_ref, is_alt = read_classes(slab)
    assert ((is_ref | is_alt).sum(axis=1) * 8 >= n).all()  # every row is deep
    exp = None
    recs = []
    for s in (slab, tag_ranks(slab)):
        for flags in (0, NO_DOM):
            got, form = lrt(bv, s, flags)
            assert form == expected_form(n, flags)
            exp = exact(restatement, got, slab, exp)
            recs.append(got)
    for r in recs[1:]:
        same(recs[0], r)
    assert_edges_hit(slab, exp[0], max_rank=255)


@pytest.mark.parametrize("G,n", [(3, 1500), (3, 12000), (3, 60000), (9, 4096), (9, 16384), (9, 60000), (20, 3000), (20, 30000),
                                 (20, 65535), (40, 5000), (40, 60000)])
def test_pop_groups(bv, restatement, G, n):
    """Pop-groups with phred 64..93 on their members' reads (the group histograms' upper halves are not empty): the streaming
    group tally (3), workgroup-per-row pass 2 (9), 16-bit group counters (20, rows of <= 65,535 samples), two rounds (40)."""
    S = min(sites_for(n), 96)
    for max_rank in (65535, 8191):
        slab = edge_slab(S, n, seed=31 * n + G + max_rank, coverage=coverage_for(n), n_groups=G, max_rank=max_rank)
        got, form = lrt(bv, slab)
        assert form == expected_form(n)
        e, g, _ = exact(restatement, got, slab)
        assert_edges_hit(slab, got, max_rank=max_rank)
        v = ranksum_sites(e)
        member = np.asarray(slab["group_id"])[:n] != 0xFF
        hiq = ((np.asarray(slab["qual"])[v, :n] >= 64) & (np.asarray(slab["base_strand"])[v, :n] < 8) & member).any(axis=1)
        assert hiq.all(), "a variant site without a phred >= 64 read of a group member"
        assert (g["total_depth"][v] > 0).sum() >= v.size * G // 2
        if max_rank <= 8191:
            same(got, lrt(bv, tag_ranks(slab))[0])


def chained(bv, slabs, layout, groups):
    """bv_engine_submit_many_g of device-resident slabs: (records per slab, BV_FORM_* bits)."""
    import torch
    dev = torch.device("cuda", 0)
    n, P = slabs[0]["n_samples"], slabs[0]["pitch"]
    eng = bv.BaseTypeEngine(max_sites=sum(s["n_sites"] for s in slabs), min_af_value=bv.min_af(n), device=0)
    keep, segs, outs, gouts = [], [], [], []
    for sl in slabs:
        s = tag_ranks(sl) if layout else sl
        t = [torch.from_numpy(np.ascontiguousarray(s[k])).to(dev) for k in ("base_strand", "qual", "ref_base", "mapq")]
        t.append(torch.from_numpy(np.ascontiguousarray(s["rpr"]).view(np.int16)).to(dev))
        out = torch.zeros(sl["n_sites"] * bv.SITE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        gout = torch.zeros(max(1, sl["n_sites"] * groups * bv.GROUP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        keep.append(t); outs.append(out); gouts.append(gout)
        segs.append((sl["n_sites"], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), out.data_ptr(), t[3].data_ptr(), t[4].data_ptr()))
    gid = torch.from_numpy(np.ascontiguousarray(slabs[0]["group_id"])).to(dev) if groups else None
    torch.cuda.synchronize()
    try:
        eng.submit_many_ptrs(n, P, segs, group_id=gid.data_ptr() if groups else 0, n_groups=groups,
                             gouts=[g.data_ptr() for g in gouts] if groups else None, layout=layout)
        form = eng.last_launch_form()
        eng.wait()
    finally:
        eng.close()
    res = []
    for sl, out, gout in zip(slabs, outs, gouts):
        sites = out.cpu().numpy().view(bv.SITE_DTYPE).copy()
        grp = gout.cpu().numpy()[:sl["n_sites"] * groups * bv.GROUP_DTYPE.itemsize].view(bv.GROUP_DTYPE).reshape(sl["n_sites"], groups) if groups else None
        res.append(BaseTypeBatch(sites, grp, int(((sites["status"] & 2) != 0).sum()), 0.0, 0.0))
    return res, form


@pytest.mark.parametrize("n,groups", [(2048, 0), (16384, 3), (70000, 0)])
def test_chained_submit_of_three_slabs(bv, restatement, n, groups):
    """Three slabs as ONE launch per pass (bv_engine_submit_many_g): every slab's records the oracle's and those of its own
    submit, byte for byte; plain ranks up to 65,535, and the tagged layout of slabs whose ranks stop at 8,191."""
    S = sites_for(n)
    for max_rank in (65535, 8191):
        slabs = [edge_slab(s, n, seed=900 + k + n + max_rank, coverage=coverage_for(n), n_groups=groups, max_rank=max_rank)
                 for k, s in enumerate((S // 2, 17, S))]
        for s in slabs[1:]:  # one group plane for the whole queue
            s["group_id"] = slabs[0].get("group_id")
        for layout in (0, 1) if max_rank <= 8191 else (0,):
            got, form = chained(bv, slabs, layout, groups)
            assert form == expected_form(n)
            for sl, g in zip(slabs, got):
                exact(restatement, g, sl)
                same(g, lrt(bv, tag_ranks(sl) if layout else sl)[0])
        assert_edges_hit(slabs[2], lrt(bv, slabs[2])[0], max_rank=max_rank)


def add_range_site(slab, row, n_cells, seed):
    """Makes `row` hold n_cells REF reads of ranks >= 8,192 (beyond the per-site tallies' window and an announced 8,191)."""
    rng = np.random.default_rng(seed)
    n = slab["n_samples"]
    _, is_alt = read_classes(slab)
    cells = rng.permutation(np.nonzero(~is_alt[row])[0])[:n_cells]
    assert cells.size == n_cells
    slab["base_strand"][row, cells] = slab["ref_base"][row] | (rng.integers(0, 2, cells.size) << 2).astype(np.uint8)
    slab["qual"][row, cells] = rng.integers(20, 41, cells.size)
    slab["mapq"][row, cells] = rng.choice([0, 60, 255], cells.size)
    slab["rpr"][row, cells] = rng.choice([8192, 16384, 32767, 65535], cells.size)
    assert n > n_cells


TILE_MODES = {
    "joined_dense": (0, {}),
    "joined_packed_batched": (0, dict(packed=True, sparse_batch=4)),
    "per_site_dense": (TILE_STATE, {}),
    "per_site_max_rank": (TILE_STATE, dict(max_rank=8191)),
    "per_site_packed_batched": (TILE_STATE, dict(packed=True, sparse_batch=3)),
    "per_site_mixed_max_rank": (TILE_STATE, dict(packed=3, max_rank=8191)),
}


@pytest.mark.parametrize("mode", sorted(TILE_MODES))
@pytest.mark.parametrize("n,width", [(2048, 512), (16384, 2000), (70000, 5000)])
def test_tile_jobs(bv, restatement, n, width, mode):
    """Sample-axis tile jobs with three pop-groups: joined rows (byte-identical to the row submit) and per-site tallies
    (agree with the oracle to 1e-6), dense, packed and batched packed tiles, with and without an announced read length.
    Rows of 16,384 samples and more hold one site with more than 2,048 ranks beyond the window: the per-site tallies must
    flag BV_SITE_RPR_RANGE with a NaN ReadPosRankSum there and nowhere else."""
    flags, kw = TILE_MODES[mode]
    S = sites_for(n)
    slab = edge_slab(S, n, seed=4400 + n, coverage=coverage_for(n), n_groups=3)
    special = None
    if n > 4096:
        special = 3  # a site of the 0.45 AF class
        add_range_site(slab, special, 2300, seed=n)
    maf = bv.min_af(n)
    exp = oracle_run(restatement, slab, maf, n_threads=16)
    e = exp[0]
    assert ((e["status"] & 2) != 0).sum() >= S // 2
    eng = bv.BaseTypeEngine(max_sites=S, min_af_value=maf, device=0, flags=flags)
    try:
        t = eng.lrt_tiles(slab, width, **kw)
    finally:
        eng.close()
    rr = (t.sites["status"] & RPR_RANGE) != 0
    if flags & TILE_STATE and special is not None:
        assert e["status"][special] & 2
        assert np.nonzero(rr)[0].tolist() == [special]
        assert np.isnan(t.sites["rpr_ranksum"][special]) and not np.isnan(e["rpr_ranksum"][special])
        sites = t.sites.copy()
        sites["rpr_ranksum"][special] = e["rpr_ranksum"][special]  # the one value that realisation does not give
        t = BaseTypeBatch(sites, t.groups, t.n_variant, 0.0, 0.0)
    else:
        assert not rr.any()
    exact(restatement, t, slab, exp)
    if flags == 0:
        same(lrt(bv, slab)[0], t)
    assert_edges_hit(slab, e)


@pytest.mark.parametrize("n,files,groups", [(60, [60], 0), (2048, [512] * 4, 0), (16384, [2000] * 8 + [384], 3), (70000, [5000] * 14, 0)],
                         ids=["60", "2048", "16384_groups", "70000"])
def test_text_rows(bv, restatement, n, files, groups):
    """The edge slabs as batchfile text: mapq, rank and quality tokens span 0..255, 0..65,535 and '!'..'~'.  No position
    goes to the host reader, the records are lrt()'s and the oracle's, the cell and phred planes come back as the slab's
    (ranks up to 65,535: plain; up to 8,191: the engine tags them)."""
    for max_rank in (65535, 8191):
        slab = edge_slab(sites_for(n), n, seed=6100 + n + max_rank, coverage=coverage_for(n), n_groups=groups, max_rank=max_rank)
        got = text_check(slab, files, n_groups=groups)  # no host position, == lrt() byte for byte, planes returned
        keep = got.positions.astype(np.int64)
        sub = {k: (v[keep] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == slab["n_sites"] and k != "group_id" else v)
               for k, v in slab.items()}
        sub["n_sites"] = int(keep.size)
        exact(restatement, got, sub)
        assert_edges_hit(sub, got, max_rank=max_rank)
