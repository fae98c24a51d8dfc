"""CPU tests (no GPU) of the allele-domain slabs (tests/allele_domain.py): the inputs that test_gpu_allele_domain.py holds
the engine to must be what they claim, by the oracle's records alone.

For every row length of ROWS and every bin class: the restatement's n_em and ALT tuple are the declared ones at every site
and every leaf of the LRT's decision tree occurs; every site's decision margin is 1e-6 * max(1, |chi2|) or more; the
threshold pair comes back with its base active (6 EM runs) and not active (3); the chi2 bracket comes back with no ALT and
with one.  Where the real reference is built it gives the restatement's records on these slabs.

Measured with the restatement (seed 1000 + class index, all six classes per row length): the smallest margin relative to
max(1, |chi2|), the relative gap to min_af of depth / total of the threshold pair (on, one read below), and the distance
of the bracket's two chi2 values from 24 (the smallest and largest seen over the classes).

    n      margin    on        below     bracket below   bracket above
    60     0.00067   2.3       1         0.264..5.54     0.654..7.22
    1500   0.00061   2.2e-08   0.33      0.401..4.8      0.28..7.11
    2048   0.00033   2.2e-08   0.25      0.0983..2.59    0.129..3.2
    2049   0.00049   2.2e-08   0.25      0.206..3.55     1.01..4.89
    4096   0.00021   2.2e-08   0.12      0.138..2.67     0.102..2.32
    4097   0.00049   2.2e-08   0.25      0.259..2.08     0.0951..2.13
    16384  7.9e-05   0         0.04      0.00523..2.96   0.39..2.1
    16385  9.1e-05   0.00031   0.1       0.0315..3.18    0.0273..2.74
    49152  2.3e-05   4.1e-05   0.12      0.318..3.45     0.0721..2.31
    49153  2.7e-05   6.1e-05   0.12      0.107..2.31     0.51..2.23
    70000  2.3e-05   1.1e-08   0.12      0.414..2.61     0.454..1.45
"""
import numpy as np
import pytest

import oracle
from allele_domain import (BIN_ORDER, LRT_THRESHOLD, ROWS, allele_slab, assert_classes, assert_leaves_hit, assert_margins,
                           oracle_records)
from test_oracle_cpu import EXACT_SKIP, assert_bit_equal


def seed_for(bins):
    return 1000 + BIN_ORDER.index(bins)


@pytest.mark.parametrize("bins", BIN_ORDER)
@pytest.mark.parametrize("n", ROWS)
def test_every_leaf_is_reached_with_a_margin(restatement, n, bins):
    slab, declared = allele_slab(n, seed_for(bins), bins, restatement=restatement)
    e, _, margins = oracle_records(restatement, slab)
    assert_leaves_hit(declared, e)
    assert_margins(margins, e)
    assert_classes(declared, n)
    maf = restatement.min_af(n)
    by = {d["name"]: (s, d) for s, d in enumerate(declared)}
    # the threshold pair: the base on the bound is active (three bases: 6 EM runs), one read below it is not (two: 3)
    s, d = by["threshold_on"]
    assert d["depth"] / d["total"] >= maf and e["n_em"][s] == 6 and sorted(e["depth"][s])[1] == d["depth"]
    s, d = by["threshold_below"]
    assert d["depth"] / d["total"] < maf and e["n_em"][s] == 3 and sorted(e["depth"][s])[1] == d["depth"]
    if n == 16384:
        assert (d["total"], d["depth"]) == (4096, 24) and by["threshold_on"][1]["gap"] == 0.0  # 25 / 4096 == min_af exactly
    # the bracket: the closest chi2 below 24 keeps no ALT, the closest above keeps one
    s, d = by["bracket_below"]
    assert e["chi2"][s] < LRT_THRESHOLD and e["n_alt"][s] == 0 and e["n_em"][s] == 3
    s, d = by["bracket_above"]
    assert e["chi2"][s] >= LRT_THRESHOLD and e["n_alt"][s] == 1 and e["n_em"][s] == 3


@pytest.mark.parametrize("n,groups", [(1500, 3), (12000, 9), (60000, 40)])
def test_built_pop_groups_call_what_is_declared(restatement, n, groups):
    """The built group compositions: the proportional share and the ALT carriers call the site's ALTs, the REF carriers
    and the group without a covered sample none; the small group stays at 64 covered samples or fewer."""
    slab, declared = allele_slab(n, 7 * n + groups, BIN_ORDER, n_groups=groups, restatement=restatement)
    e, g, margins = oracle_records(restatement, slab)
    assert_leaves_hit(declared, e, g)
    assert_margins(margins, e)
    var = (e["status"] & 2) != 0
    assert (g["total_depth"][var, 0] > 0).all() and (g["total_depth"][var, 1] > 0).all()
    assert (g["total_depth"][var, 2] > 0).any() and (g["n_alt"][var, 2] == 0).all()
    if groups > 4:
        assert (g["total_depth"][:, 3] == 0).all()
        assert (g["total_depth"][:, 4] <= 64).all() and (g["total_depth"][var, 4] > 0).any()


@pytest.mark.parametrize("n", [60, 1500, 4097, 70000])
def test_restatement_matches_reference_on_the_allele_slabs(reference, n):
    """The real reference gives the restatement's records on these slabs (the comparison of test_oracle_cpu.py)."""
    res = oracle.Restatement()
    slab, declared = allele_slab(n, 2000 + n, BIN_ORDER, n_groups=3 if n == 1500 else 0, restatement=res)
    maf = res.min_af(n)
    a, ga = res.run(slab, maf, n_threads=4)
    b, gb = reference.run(slab, maf, n_threads=4)
    assert_bit_equal(a, b, skip=EXACT_SKIP)
    if ga is not None:
        assert_bit_equal(ga, gb)
    assert_leaves_hit(declared, a, ga)
