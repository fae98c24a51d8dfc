"""GPU tests (-m gpu) over the EM loop's stopping rule (tests/em_domain.py): sites whose longest EM run takes 1, 2, 3, 4
and 5 loop passes; the loop in the top EM, in a subset EM one level down (3 -> 2, 4 -> 3), in the two-base form and in the
closed form of a single-base subset either side of 1/e; REF kept, dropped and N; a class whose first-pass log-marginal
moves by just under 1, by 1 and by 2 and more, shrinking and growing (the slivers between the (0.37, 2.7) window of the
bin-based bodies and e); every bin class, a phred-0 read (the generic body) and <= 64 covered samples (the per-sample
replay) -- through every kernel form a row length selects, the diagnostic forms, pop-groups of 3, 9 and 40 whose own calls
loop twice and more, tile jobs in both realisations and a chained submit.

Every record is held to the oracle with its margins, no site may be excused as a tie, and em_iters and n_em -- the number
of loop passes and of EM runs -- must be the oracle's exactly.  Every form reports both as the oracle does.

What the file is for, measured on MI355X with five one-line changes of the kernels, each run once over the tests at 1,500
and 4,097 samples of this file, of test_gpu_value_domain.py and of test_gpu_allele_domain.py (no test of the latter two
failed under any of them):

    change                                                   tests of this file that fail
    2.7 -> 3.0 in bv_em_wave                                 test_diagnostic_forms[wave_solver-1500-groups] (em_iters of the
                                                             sites whose marginals grow by just over e)
    0.37 -> 0.30 in bv_em_g16, general body                  test_row_lengths_loop_as_the_oracle_does[1500], [4097],
                                                             test_diagnostic_forms[short_row_form_9-4097] (af, qual, qd, chi2)
    0.37 -> 0.30 in bv_em_g16, two-base body                 none at these two lengths: only the pop-group solve kernel holds
                                                             the body; test_pop_groups_that_loop[3-*] and [9-*] (group af)
    k <= 100 -> k <= 2 in bv_em_wave_generic                 the two row lengths, wave_solver-1500-groups, short_row_form_9-4097
    the single-base subset's `it` fixed at 1                 the same four (em_iters of every site that reaches such a subset)"""
import numpy as np
import pytest

import basevar_amd

pytestmark = pytest.mark.gpu

from em_domain import assert_em_classes_hit, assert_margins, em_slab, oracle_records
from test_gpu_parity import bv  # noqa: F401  (the module fixture)
from test_gpu_tagged import same
from test_gpu_value_domain import ROWS, TILE_STATE, WAVE_SOLVER, chained, exact, expected_form, long_row_form, lrt, short_row_form

ZERO_FREQ = 0x8  # BV_SITE_ZERO_FREQ

_built = {}


def built(restatement, n, seed, groups=0):
    """(slab, declared, the oracle's (records, group records, margins)): built and solved by the oracle once per session,
    shared and left unchanged.  The inputs' own conditions are asserted here, once."""
    key = (n, seed, groups)
    if key not in _built:
        slab, declared = em_slab(n, seed, n_groups=groups, restatement=restatement)
        exp = oracle_records(restatement, slab)
        assert_em_classes_hit(declared, exp[0], n, groups)
        assert_margins(exp[2], exp[0])
        assert len(declared) <= 96
        _built[key] = (slab, declared, exp)
    return _built[key]


def hold(restatement, got, slab, declared, exp):
    """got == the oracle's records with no site excused, and the engine counts the oracle's loop passes and EM runs at
    every site (but those the reference would have thrown at)."""
    exact(restatement, got, slab, exp)
    e = exp[0]
    ok = (e["status"] & ZERO_FREQ) == 0
    for f in ("em_iters", "n_em"):
        bad = np.nonzero(ok & (got.sites[f] != e[f]))[0]
        assert bad.size == 0, "%s differs at sites %s: %s, the oracle's %s (%s)" % (
            f, bad[:8].tolist(), got.sites[f][bad[:8]].tolist(), e[f][bad[:8]].tolist(), [declared[s]["want"] for s in bad[:8]])


@pytest.mark.parametrize("n", ROWS)
def test_row_lengths_loop_as_the_oracle_does(bv, restatement, n):
    """Default flags, one row length per kernel form (rows of 49,153 and 70,000 samples: the long-row kernel's team form,
    which launches of up to 65,536 sites take)."""
    slab, declared, exp = built(restatement, n, seed=n)
    got, form = lrt(bv, slab)
    assert form == expected_form(n), "form 0x%x" % form
    hold(restatement, got, slab, declared, exp)


@pytest.mark.parametrize("flags,n,groups,identical", [
    pytest.param(WAVE_SOLVER, 1500, 3, False, id="wave_solver-1500-groups"),
    pytest.param(WAVE_SOLVER, 16384, 3, False, id="wave_solver-16384-groups"),
    pytest.param(short_row_form(9), 4097, 0, True, id="short_row_form_9-4097"),
    pytest.param(short_row_form(9), 49152, 0, True, id="short_row_form_9-49152"),
    pytest.param(short_row_form(10), 16385, 0, True, id="short_row_form_10-16385"),
    pytest.param(long_row_form(2), 49153, 0, True, id="long_row_form_2-49153"),
    pytest.param(long_row_form(2), 70000, 0, True, id="long_row_form_2-70000"),
])
def test_diagnostic_forms(bv, restatement, flags, n, groups, identical):
    """Every form meets the oracle and counts its passes; where the diag header says records do not depend on the flag, they
    are the default path's byte for byte."""
    slab, declared, exp = built(restatement, n, seed=n + 17, groups=groups)
    got, form = lrt(bv, slab, flags)
    assert form == expected_form(n, flags), "form 0x%x" % form
    hold(restatement, got, slab, declared, exp)
    if identical:
        same(lrt(bv, slab)[0], got)


@pytest.mark.parametrize("n", [3000, 12000, 60000])
@pytest.mark.parametrize("G", [3, 9, 40])
def test_pop_groups_that_loop(bv, restatement, G, n):
    """Three groups take a fixed share of every kind of read, so their own lrt([REF] + alts) loops twice and more: groups
    of <= 16 bins, <= 64 bins and more, and one of <= 64 covered samples (asserted by built()); one short, one fused and one
    long row length: the streaming tally with the 16-lane solver (3), the 4- and 8-lane solvers (9, 40), two rounds (40)."""
    slab, declared, exp = built(restatement, n, seed=7 * n + G, groups=G)
    got, form = lrt(bv, slab)
    assert form == expected_form(n)
    hold(restatement, got, slab, declared, exp)
    g = exp[1]
    var = (exp[0]["status"] & 2) != 0
    assert (g["total_depth"][var, :3] > 0).all() and (g["total_depth"][:, 2] <= 64).all()


@pytest.mark.parametrize("flags,packed", [(0, False), (0, True), (TILE_STATE, False), (TILE_STATE, True)],
                         ids=["joined_dense", "joined_packed", "per_site_dense", "per_site_packed"])
@pytest.mark.parametrize("n,width", [(2048, 512), (16384, 2000)])
def test_tile_jobs(bv, restatement, n, width, flags, packed):
    """Sample-axis tile jobs with the three built pop-groups: joined rows (byte-identical to the row submit) and the
    per-site-tally finish, which has solver call sites of its own; dense and packed tiles."""
    slab, declared, exp = built(restatement, n, seed=4400 + n, groups=3)
    eng = bv.BaseTypeEngine(max_sites=slab["n_sites"], min_af_value=bv.min_af(n), device=0, flags=flags)
    try:
        t = eng.lrt_tiles(slab, width, packed=packed)
    finally:
        eng.close()
    hold(restatement, t, slab, declared, exp)
    if flags == 0:
        same(lrt(bv, slab)[0], t)


def test_chained_submit_of_three_slabs(bv, restatement):
    """Three slabs of different seeds as ONE launch per pass: every slab's records the oracle's and those of its own submit,
    byte for byte."""
    n = 16384
    sets = [built(restatement, n, seed=900 + k + n) for k in range(3)]
    got, form = chained(bv, [s[0] for s in sets], 0, 0)
    assert form == expected_form(n)
    for (slab, declared, exp), g in zip(sets, got):
        hold(restatement, g, slab, declared, exp)
        same(g, lrt(bv, slab)[0])
