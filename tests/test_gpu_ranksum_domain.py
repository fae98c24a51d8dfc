"""GPU tests (-m gpu) of MQRankSum, ReadPosRankSum, BaseQRankSum and QUAL on sites built at a chosen z and a chosen chi2
(tests/ranksum_domain.py), through every realisation of the rank sum: the window sums of the pass-2 kernels and of the
fused kernel's rank-sum rows, the 16-value windows of the 16-lane solver, the wave and long-row solvers, the tile finish
with its rank window and pool, the finish that forms the phreds of 64 sites at once -- z exactly 0, both erfc branches on
either side of 10 / sqrt 2, the cut at 37 from both sides, complete separation, sites without a REF read, lopsided rows,
values in one window, in the first and last window, across window edges -- and QUAL where p is small, denormal and 0.

Every record is held to the oracle with the margins of tests/parity.py and no site may be excused as a tie; that the
oracle's phreds are the model's, and what the corpus of a row length populates, is asserted on the oracle's records in
tests/test_ranksum_domain_cpu.py.

No corpus entry found a difference: every form gave the oracle's records.  What the module is sensitive to was measured
with two one-line changes of the library, each in a build of its own: the erfc cut at 36 instead of 37 fails 26 of the 30
tests (all but rows of 60 and 1,500 samples, which cannot reach |z| = 36: the "below_cut" sites, 10000 for about 2,970), and
`- t` for `- t + 1` in bv_ranksum_window_g16 alone fails the 22 that meet the 16-lane solver (every test on short rows of
more than 64 covered reads; the eight that pass run rows of 60 samples or the long-row kernel)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ranksum_domain as rd
from basevar_amd.engine import BaseTypeBatch
from basevar_amd.synth import tag_ranks
from test_gpu_parity import bv, check, oracle_run  # noqa: F401  (bv: the module fixture)
from test_gpu_tagged import same
from test_gpu_text_rows import check as text_check
from test_gpu_value_domain import (NO_DOM, P2_TAIL_DMA, PASS2_SWEEP, RPR_RANGE, TILE_STATE, WAVE_SOLVER, expected_form,
                                   long_row_form, lrt, short_row_form)

ROWS = (60, 1500, 2048, 4096, 4097, 16385, 49152, 49153, 70000)
RANK_FIELDS = tuple(rd.FIELD[s] for s in rd.STATS)
_built = {}


def built(restatement, n, max_rank=65535, groups=0):
    """(sites, slab, the oracle's (records, group records, margins)) of the corpus and the QUAL sites of a row length in
    identity order: built and solved by the oracle once per session, shared and left unchanged."""
    key = (n, max_rank, groups)
    if key not in _built:
        sites = list(rd.corpus(n, max_rank)) + rd.qual_sites(restatement, n)[0]
        slab = rd.slab(sites, n)
        if groups:
            gid = np.random.default_rng([n, groups]).integers(0, groups, n).astype(np.uint8)
            gid[np.random.default_rng([n, groups, 1]).random(n) < 0.1] = 0xFF   # one sample in ten in no group
            slab["group_id"], slab["n_groups"] = gid, groups
        exp = oracle_run(restatement, slab, restatement.min_af(n), n_threads=16)
        assert ((exp[0]["status"] & 0x12) == 0x12).all()
        _built[key] = (sites, slab, exp)
    return _built[key]


def hold(got, exp):
    e, g, margins = exp
    assert check(got, e, g, margins) == 0, "a site needed the tie excuse"


def zeros_keep_their_sign(got, exp):
    """A z of exactly 0 is -10 log10(1.0): the zero's sign bit is the oracle's, in all three fields."""
    e = exp[0]
    n_zero = 0
    for f in RANK_FIELDS:
        zero = e[f] == 0.0
        n_zero += int(zero.sum())
        assert np.array_equal(np.signbit(got.sites[f][zero]), np.signbit(e[f][zero])), f
    assert n_zero >= len(e)   # (two fields of nearly every site: the statistics not under test)


def classes_as_the_oracle(sites, got, exp):
    """What the engine's records populate is what the oracle's do: every |z| class, 10000 beyond the cut and without a REF
    read, the QUAL ranges and the exact zero of p."""
    for site, g, e in zip(sites, got.sites, exp[0]):
        assert rd.labels(site, g) == rd.labels(site, e), site["name"]


def reordered(exp, order):
    e, g, margins = exp
    return e[order], None if g is None else g[order], margins[order]


@pytest.mark.parametrize("n", ROWS)
def test_corpus_through_every_row_form(bv, restatement, n):
    """The corpus and the QUAL sites of each row length through the kernels that row length selects: the per-sample replay
    (60), the three launches with either pass 2 (<= 4,096 samples), the fused kernel (<= 49,152), the long-row kernel.  The
    QUAL sites meet the 16-lane solver, the wave solver (60 samples: shallow sites) and the long-row solver.  The corpus
    whose ranks stop at 8,191 gives the oracle's records too, and in the tagged layout the plain layout's byte for byte."""
    sites, slab, exp = built(restatement, n)
    got, form = lrt(bv, slab)
    assert form == expected_form(n), "form 0x%x" % form
    hold(got, exp)
    zeros_keep_their_sign(got, exp)
    classes_as_the_oracle(sites, got, exp)
    _, slab8, exp8 = built(restatement, n, 8191)
    got8, form = lrt(bv, slab8)
    assert form == expected_form(n)
    hold(got8, exp8)
    zeros_keep_their_sign(got8, exp8)
    tagged, tform = lrt(bv, tag_ranks(slab8))
    assert tform == form
    same(got8, tagged)


@pytest.mark.parametrize("n", [1500, 16385, 70000])
def test_regimes_on_adjacent_sites(bv, restatement, n):
    """The same sites in three orders.  In the model of ranksum_domain.orders neighbours in site order sit in neighbouring lanes
    of the finish that forms 64 sites' mq and rpr phreds at once (the real assignment is the kernels' business): between them the orders put every ordered
    pair of z = 0, first erfc branch, second branch, above the cut and no REF read, of each statistic, on adjacent sites, where
    the branches of bv_kf_erfc and the early returns of bv_ranksum_phred run under divergent control flow.  Every order gives
    the oracle's records, and, the permutation undone, the identity order's byte for byte."""
    sites, slab, exp = built(restatement, n)
    orders, pairs, wanted = rd.orders(sites)
    assert pairs >= wanted
    first = None
    for order in orders:
        got, form = lrt(bv, rd.slab(sites, n, order))
        assert form == expected_form(n)
        hold(got, reordered(exp, order))
        back = np.argsort(order)
        undone = BaseTypeBatch(got.sites[back], None, got.n_variant, 0.0, 0.0)
        if first is None:
            first = undone
        same(first, undone)


@pytest.mark.parametrize("flags,n,identical", [
    pytest.param(P2_TAIL_DMA, 16384, True, id="p2_tail_dma-16384"),
    pytest.param(P2_TAIL_DMA, 49152, True, id="p2_tail_dma-49152"),
    pytest.param(short_row_form(9), 4097, True, id="short_row_form_9-4097"),
    pytest.param(short_row_form(9), 49152, True, id="short_row_form_9-49152"),
    pytest.param(short_row_form(10), 16385, True, id="short_row_form_10-16385"),
    pytest.param(PASS2_SWEEP, 2049, False, id="pass2_sweep-2049"),
    pytest.param(PASS2_SWEEP, 16384, False, id="pass2_sweep-16384"),
    pytest.param(long_row_form(2), 49153, True, id="long_row_form_2-49153"),
    pytest.param(WAVE_SOLVER, 1500, False, id="wave_solver-1500"),
    pytest.param(WAVE_SOLVER, 16384, False, id="wave_solver-16384"),
    pytest.param(NO_DOM, 2048, True, id="no_dom-2048"),
    pytest.param(NO_DOM, 70000, True, id="no_dom-70000"),
])
def test_diagnostic_forms(bv, restatement, flags, n, identical):
    """Every diagnostic form meets the oracle; where include/basevar_amd_diag.h says records do not depend on the flag, they
    are the default path's byte for byte.  Both layouts on the corpus whose ranks stop at 8,191 (the LDS-DMA rings and the
    dominant-value tally have their say on the tagged layout too).  BV_FLAG_NO_DOM: the corpus holds deep sites -- an
    eighth of the row's cells or more are REF and ALT reads -- of every regime, which is where the dominant mapq is counted."""
    for max_rank in (65535, 8191):
        sites, slab, exp = built(restatement, n, max_rank)
        if flags == NO_DOM:
            assert sum((s["n1"] + s["n2"]) * 8 >= n and s["stat"] == "mq" for s in sites) >= 5
        for s in [slab] + ([tag_ranks(slab)] if max_rank <= 8191 else []):
            base, f0 = lrt(bv, s)
            got, f1 = lrt(bv, s, flags)
            assert f0 == expected_form(n) and f1 == expected_form(n, flags), "forms 0x%x 0x%x" % (f0, f1)
            hold(got, exp)
            hold(base, exp)
            zeros_keep_their_sign(got, exp)
            if identical:
                same(base, got)


@pytest.mark.parametrize("G,n", [(3, 2048), (3, 16385), (20, 60000)])
def test_pop_groups(bv, restatement, G, n):
    """With pop-groups the rank-sum rows go through bv_pass2_kernel<.., RANKS, GROUPS>, or through the fused kernel with the
    group-only tally behind it: site and group records are the oracle's, and the site records' three rank sums are those of
    the run without groups, byte for byte."""
    sites, slab, exp = built(restatement, n, groups=G)
    got, form = lrt(bv, slab)
    assert form == expected_form(n)
    hold(got, exp)
    assert (exp[1]["total_depth"] > 0).sum() >= len(sites) * G // 2
    plain = {k: v for k, v in slab.items() if k != "group_id"}
    plain["n_groups"] = 0
    alone, _ = lrt(bv, plain)
    for f in RANK_FIELDS:
        assert got.sites[f].tobytes() == alone.sites[f].tobytes(), f
    zeros_keep_their_sign(got, exp)


def beyond_the_tile_window(sites, window=1024, listed=2048):
    """Sites with more than `listed` REF and ALT reads of a rank beyond the per-site tallies' window (csrc/bv_tiles.hip: up to
    BV_TS_OVF_LIST such reads are ranked from the pool, more give BV_SITE_RPR_RANGE and a NaN), and sites with any."""
    count = np.array([int((s["ref"]["rpr"] >= window).sum() + (s["alt"]["rpr"] >= window).sum()) for s in sites])
    return count > listed, count > 0


@pytest.mark.parametrize("n,width", [(2048, 512), (70000, 5000)])
def test_tile_jobs(bv, restatement, n, width):
    """Sample-axis tile jobs: joined rows are the row submit's records byte for byte.  The per-site-tally finish
    (BV_FLAG_TILE_STATE) has rank windows of its own: ranks below 1,024 from the window, up to 2,048 reads beyond it ranked
    from the pool -- the corpus's 1,023 | 1,024, 7 | 8,191 and 7 | 60,000 sites --, and a site with more such reads is flagged
    BV_SITE_RPR_RANGE with a NaN ReadPosRankSum, that site and no other.  Everything else is the oracle's."""
    sites, slab, exp = built(restatement, n)
    e = exp[0]
    for flags in (0, TILE_STATE):
        eng = bv.BaseTypeEngine(max_sites=slab["n_sites"], min_af_value=bv.min_af(n), device=0, flags=flags)
        try:
            t = eng.lrt_tiles(slab, width)
        finally:
            eng.close()
        rr = (t.sites["status"] & RPR_RANGE) != 0
        if flags == 0:
            assert not rr.any()
            hold(t, exp)
            same(lrt(bv, slab)[0], t)
            continue
        too_many, some = beyond_the_tile_window(sites)
        assert (some & ~too_many).sum() >= 8, "no site ranked from the pool"
        assert np.array_equal(rr, too_many), ([sites[i]["name"] for i in np.nonzero(rr != too_many)[0]])
        assert np.isnan(t.sites["rpr_ranksum"][rr]).all() and not np.isnan(e["rpr_ranksum"]).any()
        fixed = t.sites.copy()
        fixed["rpr_ranksum"][rr] = e["rpr_ranksum"][rr]   # the one value that realisation does not give
        t = BaseTypeBatch(fixed, t.groups, t.n_variant, 0.0, 0.0)
        hold(t, exp)
        zeros_keep_their_sign(t, exp)
        classes_as_the_oracle([s for s, r in zip(sites, rr) if not r], BaseTypeBatch(fixed[~rr], None, 0, 0.0, 0.0), (e[~rr],))


def test_corpus_as_text_rows(bv, restatement):
    """The corpus of 2,048 samples as batchfile text in four files of 512: every position parsed on the device, the
    records lrt()'s byte for byte, and the oracle's."""
    n = 2048
    sites, slab, exp = built(restatement, n)
    got = text_check(slab, [512] * 4)
    assert got.positions.size == slab["n_sites"]
    hold(got, exp)
    zeros_keep_their_sign(got, exp)
