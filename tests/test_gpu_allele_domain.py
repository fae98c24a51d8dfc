"""GPU tests (-m gpu) over the LRT's whole allele decision tree (tests/allele_domain.py): one to four active bases, every
chain of accept / reject decisions (1, 3, 4, 6, 5, 8 and 10 EM runs), REF kept, dropped by the LRT, without reads or N,
sites of <= 16 to > 128 (base, phred) bins and with a phred-0 read, a base on the min_af bound and one read below it, a
chi2 closest below and above 24 -- through every kernel form a row length selects, the diagnostic forms, pop-groups of
built composition from 3 to 40, chained submits, tile jobs in both realisations and batchfile text rows.

Every record is held to the oracle with its margins and no site may be excused as a tie; the oracle's records must show
every declared leaf (assert_leaves_hit), and the engine's n_em -- the leaf a site took -- must be the oracle's."""
import numpy as np
import pytest

import basevar_amd

pytestmark = pytest.mark.gpu

from basevar_amd.synth import tag_ranks
from allele_domain import BIN_ORDER, ROWS, allele_slab, assert_classes, assert_leaves_hit, assert_margins, oracle_records
from test_gpu_parity import bv  # noqa: F401  (the module fixture)
from test_gpu_tagged import same
from test_gpu_text_rows import check as text_check
from test_gpu_value_domain import ROWS as VALUE_ROWS
from test_gpu_value_domain import TILE_STATE, WAVE_SOLVER, chained, exact, expected_form, long_row_form, lrt, short_row_form

ZERO_FREQ = 0x8  # BV_SITE_ZERO_FREQ
assert ROWS == VALUE_ROWS

_built = {}


def built(restatement, n, seed, groups=0):
    """(slab, declared, the oracle's (records, group records, margins)) of a slab of all six bin classes: built and solved by
    the oracle once per session, shared and left unchanged.  The inputs' own conditions are asserted here, once."""
    key = (n, seed, groups)
    if key not in _built:
        slab, declared = allele_slab(n, seed, BIN_ORDER, n_groups=groups, restatement=restatement)
        exp = oracle_records(restatement, slab)
        assert_leaves_hit(declared, exp[0], exp[1])
        assert_margins(exp[2], exp[0])
        assert_classes(declared, n)
        _built[key] = (slab, declared, exp)
    return _built[key]


def hold(restatement, got, slab, declared, exp):
    """got == the oracle's records with no site excused, the oracle's records show every declared leaf, and the engine
    counts the oracle's EM runs at every site (but those the reference would have thrown at)."""
    exact(restatement, got, slab, exp)
    e, g, _ = exp
    assert_leaves_hit(declared, e, g)
    ok = (e["status"] & ZERO_FREQ) == 0
    bad = np.nonzero(ok & (got.sites["n_em"] != e["n_em"]))[0]
    assert bad.size == 0, "n_em differs at sites %s: %s, the oracle's %s (%s)" % (
        bad[:8].tolist(), got.sites["n_em"][bad[:8]].tolist(), e["n_em"][bad[:8]].tolist(), [declared[s]["name"] for s in bad[:8]])


@pytest.mark.parametrize("n", ROWS)
def test_row_lengths_reach_every_leaf(bv, restatement, n):
    """Default flags, one row length per kernel form; the tagged layout gives the plain layout's records byte for byte."""
    slab, declared, exp = built(restatement, n, seed=n)
    got, form = lrt(bv, slab)
    assert form == expected_form(n), "form 0x%x" % form
    hold(restatement, got, slab, declared, exp)
    tagged, tform = lrt(bv, tag_ranks(slab))
    assert tform == form
    same(got, tagged)


@pytest.mark.parametrize("flags,n,identical", [
    pytest.param(WAVE_SOLVER, 1500, False, id="wave_solver-1500"),
    pytest.param(WAVE_SOLVER, 16384, False, id="wave_solver-16384"),
    pytest.param(WAVE_SOLVER, 49152, False, id="wave_solver-49152"),
    pytest.param(short_row_form(9), 1500, True, id="short_row_form_9-1500"),
    pytest.param(short_row_form(9), 16384, True, id="short_row_form_9-16384"),
    pytest.param(short_row_form(9), 49152, True, id="short_row_form_9-49152"),
    pytest.param(short_row_form(10), 1500, True, id="short_row_form_10-1500"),
    pytest.param(short_row_form(10), 16384, True, id="short_row_form_10-16384"),
    pytest.param(short_row_form(10), 49152, True, id="short_row_form_10-49152"),
    pytest.param(long_row_form(2), 49153, True, id="long_row_form_2-49153"),
    pytest.param(long_row_form(2), 70000, True, id="long_row_form_2-70000"),
    pytest.param(1 << 16, 16384, True, id="grid_limit_1-16384"),
    pytest.param(2 << 16, 16384, True, id="grid_limit_2-16384"),
])
def test_diagnostic_forms(bv, restatement, flags, n, identical):
    """Every form meets the oracle; where the diag header says records do not depend on the flag, they are the default
    path's byte for byte."""
    slab, declared, exp = built(restatement, n, seed=n)
    got, form = lrt(bv, slab, flags)
    assert form == expected_form(n, flags), "form 0x%x" % form
    hold(restatement, got, slab, declared, exp)
    if identical:
        same(lrt(bv, slab)[0], got)


@pytest.mark.parametrize("n", [1500, 12000, 60000])
@pytest.mark.parametrize("G", [3, 9, 40])
def test_pop_groups_of_built_composition(bv, restatement, G, n):
    """A proportional share, ALT carriers only, REF carriers only, no covered sample, <= 64 covered samples, the rest split
    evenly: the streaming group tally (3), the 4- and 8-lane solvers (9, 40), two rounds (40).  The declared (n_alt, alt)
    of every (site, group) is held against the oracle's group records, the engine's group records against the oracle's."""
    slab, declared, exp = built(restatement, n, seed=7 * n + G, groups=G)
    got, form = lrt(bv, slab)
    assert form == expected_form(n)
    hold(restatement, got, slab, declared, exp)
    g = exp[1]
    var = (exp[0]["status"] & 2) != 0
    assert (g["total_depth"][var, :2] > 0).all() and (g["total_depth"][var, 2] > 0).any()
    if G > 4:
        assert (g["total_depth"][:, 3] == 0).all() and (g["total_depth"][:, 4] <= 64).all()
    same(got, lrt(bv, tag_ranks(slab))[0])


@pytest.mark.parametrize("n", [2048, 70000])
def test_chained_submit_of_three_slabs(bv, restatement, n):
    """Three slabs of different seeds as ONE launch per pass: every slab's records the oracle's and those of its own submit,
    byte for byte."""
    sets = [built(restatement, n, seed=900 + k + n) for k in range(3)]
    got, form = chained(bv, [s[0] for s in sets], 0, 0)
    assert form == expected_form(n)
    for (slab, declared, exp), g in zip(sets, got):
        hold(restatement, g, slab, declared, exp)
        same(g, lrt(bv, slab)[0])


@pytest.mark.parametrize("groups", [0, 3])
@pytest.mark.parametrize("flags,packed", [(0, False), (0, True), (TILE_STATE, False), (TILE_STATE, True)],
                         ids=["joined_dense", "joined_packed", "per_site_dense", "per_site_packed"])
@pytest.mark.parametrize("n,width", [(2048, 512), (70000, 5000)])
def test_tile_jobs(bv, restatement, n, width, flags, packed, groups):
    """Sample-axis tile jobs: joined rows (byte-identical to the row submit) and the per-site-tally finish, which has
    solver call sites of its own; dense and packed tiles; without pop-groups and with the three built ones."""
    slab, declared, exp = built(restatement, n, seed=4400 + n + groups, groups=groups)
    eng = bv.BaseTypeEngine(max_sites=slab["n_sites"], min_af_value=bv.min_af(n), device=0, flags=flags)
    try:
        t = eng.lrt_tiles(slab, width, packed=packed)
    finally:
        eng.close()
    hold(restatement, t, slab, declared, exp)
    if flags == 0:
        same(lrt(bv, slab)[0], t)


@pytest.mark.parametrize("n,files", [(60, [60]), (2048, [512] * 4)], ids=["60", "2048"])
def test_text_rows(bv, restatement, n, files):
    """The slabs as batchfile text: no position goes to the host reader, the records are lrt()'s byte for byte and the
    oracle's."""
    slab, declared, exp = built(restatement, n, seed=6100 + n)
    got = text_check(slab, files)
    assert got.positions.size == slab["n_sites"]
    hold(restatement, got, slab, declared, exp)
