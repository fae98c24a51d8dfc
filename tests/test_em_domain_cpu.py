"""CPU tests (no GPU) of the EM-domain slabs (tests/em_domain.py): the inputs that test_gpu_em_domain.py holds the engine to
must be what they claim, by the oracle's records alone.

At 60, 1,500 and 16,385 samples, without pop-groups and with three: the loop passes of the serial float64 model, summed
over a site's EM runs, are the restatement's em_iters at every site, and the model's runs its n_em; every class of
em_domain.TAGS that the row length can hold occurs (rows of <= 64 samples: all but OUT_OF_REACH_SHORT); every
llh_new - llh_old beyond 0.99 in size lies 1e-6 or more from an integer, and every oracle margin is 1e-6 * max(1, |chi2|)
or more.  Where the real reference is built it gives the restatement's records on these slabs.

Measured with the restatement (seed 3000 + n): the longest EM run the search reaches takes 5 loop passes (one strong and 500
phred-1 reads of a base beside 760 to 800 of another: 1,261 reads and more; the cap of 100 is out of reach of integer
phreds); on rows of 60 samples 2.  The largest em_iters - n_em of a site is 4 (1,500 and 16,385 samples) and 3 (60)."""
import numpy as np
import pytest

import oracle
from em_domain import MARGIN_REL, TAGS, assert_em_classes_hit, assert_margins, em_slab, oracle_records, wanted_tags
from test_oracle_cpu import EXACT_SKIP, assert_bit_equal

ROWS = [60, 1500, 16385]


@pytest.mark.parametrize("groups", [0, 3])
@pytest.mark.parametrize("n", ROWS)
def test_model_counts_the_oracles_passes(restatement, n, groups):
    slab, declared = em_slab(n, 3000 + n, n_groups=groups, restatement=restatement)
    e, g, margins = oracle_records(restatement, slab)
    assert_em_classes_hit(declared, e, n, groups)  # em_iters and n_em: the model's, at every site
    assert_margins(margins, e)
    assert min(d["trunc"] for d in declared) >= MARGIN_REL
    assert len(declared) <= 96
    info = declared[0]["slab"]
    print("n %d groups %d: %d sites, longest run %d passes, largest em_iters - n_em %d, smallest truncation margin %.3g" % (
        n, groups, len(declared), info["longest"], int((e["em_iters"].astype(int) - e["n_em"]).max()), min(d["trunc"] for d in declared)))
    assert info["longest"] >= (5 if n > 64 else 2)
    # the loop is not idle: most sites run some EM twice or more
    assert (e["em_iters"] > e["n_em"]).sum() * 2 > len(declared)
    if groups:
        var = (e["status"] & 2) != 0
        assert (g["total_depth"][var, :3] > 0).all()


def test_every_class_is_wanted_somewhere():
    assert set(wanted_tags(1500)) == set(TAGS) and set(wanted_tags(60)) < set(TAGS)


@pytest.mark.parametrize("n", ROWS)
def test_restatement_matches_reference_on_the_em_slabs(reference, n):
    """The real reference gives the restatement's records on these slabs (the comparison of test_oracle_cpu.py)."""
    res = oracle.Restatement()
    slab, declared = em_slab(n, 3100 + n, n_groups=3, restatement=res)
    maf = res.min_af(n)
    a, ga = res.run(slab, maf, n_threads=4)
    b, gb = reference.run(slab, maf, n_threads=4)
    assert_bit_equal(a, b, skip=EXACT_SKIP)
    assert_bit_equal(ga, gb)
    assert_em_classes_hit(declared, a, n, 3)
