"""GPU tests (-m gpu) of FS and SOR on strand tables built by construction (tests/strand_tables.py), through the three
realisations of the Fisher test that short rows take: the 16-lane form in its product, narrow and probed regimes, the
one-lane walk of hom-ref sites, and the wave form of shallow sites and phred-0 calls -- q underflowing to 0 and in the
denormal range, the observed table at either end of its family, ties, one-strand ALT reads, the 12 | 13, 32 | 33 and
128 | 129 boundaries, tables of different regimes in the four groups of one wave.

Every record is held to the oracle with the margins of tests/parity.py and no site may be excused as a tie; what the
corpus of a row length populates is asserted on the oracle's records in tests/test_strand_tables_cpu.py.

The corpus tables named "probed R=max q300, left / right of the mode" (q ~ 1e-300 inside a long family) are the ones
that found the seed of a probed tail underflowing to 0: the 16-lane form gave half the reference's p, the wave form
p = 0 (FS 10000), on every row length.  Both forms now carry such families scaled (bv_fisher_shift, csrc/bv_fisher.h).
The "steep end" tables (the family's first table below e^-760 beside an ordinary q) found the same zero in the wave form's
first round: FS 10000 for the reference's 0.9 at (250, 5, 15835, 295); walks now start at their first live table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import strand_tables as st
from basevar_amd.engine import BaseTypeBatch
from basevar_amd.synth import tag_ranks
from test_gpu_parity import bv, check, oracle_run  # noqa: F401  (bv: the module fixture)
from test_gpu_tagged import same
from test_gpu_text_rows import check as text_check
from test_gpu_value_domain import P2_TAIL_DMA, TILE_STATE, WAVE_SOLVER, expected_form, lrt, short_row_form

ROWS = (1500, 2048, 4096, 4097, 16385, 49152, 49153)
_built = {}


def cvg_table(t):
    t = tuple(t) + (0, 0)
    return (t[0], t[1], t[2] + t[4], t[3] + t[5])


def built(restatement, n):
    """(slab, the oracle's (records, group records, margins)) of the corpus of a row length in identity order: built and
    solved by the oracle once per session, shared and left unchanged.  What the oracle's FS / SOR must show is asserted here."""
    if n not in _built:
        C = st.corpus(n)
        slab = st.slab(C, n)
        exp = oracle_run(restatement, slab, restatement.min_af(n), n_threads=16)
        e = exp[0]
        for i, t in enumerate(C):
            cv = cvg_table(t)
            assert tuple(e["cvg_sb"][i]) == cv
            if st.family(cv)[0] != st.family(cv)[1] and st.log10_q(cv) < st.ZERO_LOG10:
                assert e["cvg_fs"][i] == 10000.0, C.names[i]
            if cv[1] == 0 or cv[2] == 0:
                assert e["cvg_sor"][i] == 10000.0, C.names[i]
        assert ((e["cvg_fs"] > 2900) & (e["cvg_fs"] < 3300)).any()   # q next to the smallest double, and p not 0
        _built[n] = (slab, exp)
    return _built[n]


def hold(got, exp):
    e, g, margins = exp
    assert check(got, e, g, margins) == 0, "a site needed the tie excuse"


def reordered(exp, order):
    e, g, margins = exp
    return e[order], None if g is None else g[order], margins[order]


@pytest.mark.parametrize("n", ROWS)
def test_tables_through_every_row_form(bv, restatement, n):
    """The corpus of each row length through the kernels that row length selects: the three launches (<= 4,096 samples), the
    fused kernel (<= 49,152) and, at 49,153, the long-row kernel at its shortest row -- whose wave form already has a
    by-construction test (test_gpu_parity.test_fisher_regimes_by_construction)."""
    slab, exp = built(restatement, n)
    got, form = lrt(bv, slab)
    assert form == expected_form(n), "form 0x%x" % form
    hold(got, exp)


@pytest.mark.parametrize("n", [1500, 16385])
def test_regimes_share_a_wave(bv, restatement, n):
    """The same sites in four orders.  In the model of strand_tables.wave_slots candidates are packed four to a wave in site
    order (the <= 2-active and the 3+-active lists each on its own; the real order across waves may differ): between them the orders put a product, a narrow, a probed and a degenerate table and one whose q
    is 0 into each of the four 16-lane groups, and every ordered pair of them into neighbouring groups of one wave -- where
    the row-local sums, ballots and broadcasts run under divergent control flow and the blocks differ in length.  Every
    order gives the oracle's records, and the identity order's byte for byte."""
    C = st.corpus(n)
    slab, exp = built(restatement, n)
    orders, slots, pairs = st.wave_orders(C, n, restatement.min_af(n))
    assert slots >= {(k, s) for k in st.WAVE_KINDS for s in range(4)}
    assert pairs >= {(a, b) for a in st.WAVE_KINDS for b in st.WAVE_KINDS}
    assert np.array_equal(orders[0], np.arange(len(C))) and np.array_equal(orders[1], np.arange(len(C))[::-1])
    first = None
    for order in orders:
        got, form = lrt(bv, st.slab(C, n, order))
        assert form == expected_form(n)
        hold(got, reordered(exp, order))
        back = np.argsort(order)
        undone = BaseTypeBatch(got.sites[back], None, got.n_variant, 0.0, 0.0)
        if first is None:
            first = undone
        same(first, undone)


def with_wave_solver_sites(restatement, n):
    """The corpus plus four sites that keep the one-site-per-wave solver on short rows without any flag: two of at most 64
    covered reads, two (one variant, one hom-ref) in which one ALT read has phred 0."""
    key = (n, "wave")
    if key not in _built:
        C = st.corpus(n)
        maf = restatement.min_af(n)
        hom_ref = (700, 680, 3, 2)
        extra = [(32, 0, 0, 32), (20, 12, 3, 29), (300, 280, 40, 20), hom_ref]
        tables = list(C) + extra
        slab = st.slab(tables, n)
        for t, phred0 in zip(extra, (False, False, True, True)):
            assert st.classify(t, n, maf, phred0=phred0)["solver"] == "wave"
        assert st.classify(hom_ref, n, maf)["solver"] == "lane"   # ... which only the phred-0 call changes
        for site in (len(C) + 2, len(C) + 3):
            t = tables[site]
            slab["qual"][site, t[0] + t[1]] = 0     # the first ALT read
        _built[key] = (slab, oracle_run(restatement, slab, maf, n_threads=16))
    return _built[key]


@pytest.mark.parametrize("n", [1500, 16385])
def test_wave_solver_and_flags(bv, restatement, n):
    """Every candidate on the one-site-per-wave solver (BV_FLAG_WAVE_SOLVER), the three launches and the fused kernel with a
    pass 2 of its own (BV_FLAG_SHORT_ROW_FORM 9 and 10), the rank-sum rows through the LDS-DMA rings (BV_FLAG_P2_TAIL_DMA):
    all the oracle's; where include/basevar_amd_diag.h says records do not depend on the flag, the default path's byte for
    byte."""
    slab, exp = with_wave_solver_sites(restatement, n)
    base, form = lrt(bv, slab)
    assert form == expected_form(n)
    hold(base, exp)
    for flags, identical in ((WAVE_SOLVER, False), (short_row_form(9), True), (short_row_form(10), True), (P2_TAIL_DMA, True)):
        got, form = lrt(bv, slab, flags)
        assert form == expected_form(n, flags), "flags 0x%x: form 0x%x" % (flags, form)
        hold(got, exp)
        if identical:
            same(base, got)
    # (plain ranks always take the rings: the flag has its say on the tagged layout)
    tagged = tag_ranks(slab)
    got, _ = lrt(bv, tagged, P2_TAIL_DMA)
    hold(got, exp)
    same(lrt(bv, tagged)[0], got)
    same(base, got)


def test_tables_in_tile_jobs(bv, restatement):
    """Sample-axis tile jobs of width 512 at 2,048 samples: joined rows are the row submit's records byte for byte; the
    per-site-tally finish has Fisher call sites of its own and is held to the oracle."""
    n = 2048
    slab, exp = built(restatement, n)
    for flags in (0, TILE_STATE):
        eng = bv.BaseTypeEngine(max_sites=slab["n_sites"], min_af_value=bv.min_af(n), device=0, flags=flags)
        try:
            t = eng.lrt_tiles(slab, 512)
        finally:
            eng.close()
        hold(t, exp)
        if flags == 0:
            same(lrt(bv, slab)[0], t)


def test_tables_as_text_rows(bv, restatement):
    """The corpus of 2,048 samples as batchfile text in four files of 512: every position parsed on the device, the
    records lrt()'s byte for byte, and the oracle's."""
    n = 2048
    slab, exp = built(restatement, n)
    got = text_check(slab, [512] * 4)
    assert got.positions.size == slab["n_sites"]
    hold(got, exp)
