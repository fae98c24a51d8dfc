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
first round: FS 10000 for the reference's 0.9 at (250, 5, 15835, 295); walks now start at their first live table.

Long rows (the second half of this file) take the wave form on every site: the corpora of 100,000 and 140,000 samples and
the list of 1,000,000 (strand_tables.corpus_long, corpus_million) hold its own boundaries -- 64 | 65 and 256 | 257 tables,
probe spans 62 | 63 | 64, windows of a hundred rounds, a shifted family whose window starts below the live floor after a
probe, log-factorial arguments on both sides of the table's end -- and the products of SOR around 2^31 and 2^32.  The
tables "SOR den 65536 x 65536" (and 524288 x 8192 at a million samples) found SOR = inf and nan where the reference as
compiled writes 10000: its guard is "the wrapped denominator is not 0" (bv_strand_bias_tail, csrc/bv_fisher.h)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import strand_tables as st
from basevar_amd.engine import BaseTypeBatch
from basevar_amd.synth import tag_ranks
from test_gpu_parity import bv, check, oracle_run  # noqa: F401  (bv: the module fixture)
from test_gpu_tagged import same
from test_gpu_text_rows import check as text_check
from test_gpu_value_domain import P2_TAIL_DMA, TILE_STATE, WAVE_SOLVER, expected_form, long_row_form, lrt, short_row_form

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


# ------------------------------------------------------------------------------------------------ long rows: the wave form
SOR_OVERFLOW = 0x20  # BV_SITE_SOR_OVERFLOW


def built_long(restatement, n, tables=None, key=None):
    """(corpus, slab, the oracle's (records, group records, margins)) of a long corpus (or of `tables` at n samples, cached
    under `key`): built and solved by the oracle once per session, shared and left unchanged."""
    key = key or n
    if key not in _built:
        C = tables if tables is not None else st.corpus_million() if n == st.MILLION else st.corpus_long(n)
        slab = st.slab(C, n)
        exp = oracle_run(restatement, slab, restatement.min_af(n), n_threads=16)
        e = exp[0]
        wrapped = 0
        for i, t in enumerate(C):
            cv = cvg_table(t)
            assert tuple(e["cvg_sb"][i]) == cv
            if cv[1] * cv[2] % 2 ** 32 == 0:    # an empty cell, or a product that wraps to 0: no division
                assert e["cvg_sor"][i] == 10000.0, t
                wrapped += cv[1] * cv[2] > 0
            assert bool(e["status"][i] & SOR_OVERFLOW) == (st.overflows(cv) or (e["n_alt"][i] > 0 and st.overflows(tuple(int(x) for x in e["var_sb"][i])))), t
        assert wrapped >= (1 if n >= 133072 and tables is None else 0)
        assert np.isfinite(e["cvg_sor"]).all()
        _built[key] = (C, slab, exp)
    return _built[key]


def hold_long(got, exp):
    """The oracle's records, no site excused as a tie, and BV_SITE_SOR_OVERFLOW the oracle's on every site (which the
    status mask of tests/parity.py leaves out)."""
    hold(got, exp)
    assert np.array_equal(got.sites["status"] & SOR_OVERFLOW, exp[0]["status"] & SOR_OVERFLOW), \
        np.nonzero((got.sites["status"] ^ exp[0]["status"]) & SOR_OVERFLOW)[0].tolist()


@pytest.mark.parametrize("n", st.LONG_ROWS)
def test_long_tables_with_and_without_the_team_tail(bv, restatement, n):
    """The long corpora through the long-row kernel.  With ~150 sites every deep site of the default launch is a team job: its
    Fisher tests run on a helper wave, the VCF table crossing to it through the team's shared block (csrc/bv_pass1_team.h);
    under BV_FLAG_LONG_ROW_FORM(2) the solver wave runs them alone.  Both the oracle's records, and each other's byte for byte."""
    C, slab, exp = built_long(restatement, n)
    base, form = lrt(bv, slab)
    assert form == expected_form(n), "form 0x%x" % form
    hold_long(base, exp)
    alone, form = lrt(bv, slab, long_row_form(2))
    assert form == expected_form(n)
    hold_long(alone, exp)
    same(base, alone)


@pytest.mark.parametrize("n", st.LONG_ROWS)
def test_long_tables_beyond_the_log_factorial_table(bv, restatement, n):
    """An engine created for 1,000 samples keeps a log-factorial table of 65,536 entries: every argument beyond it takes the
    series, and the tables whose cells lie on both sides of 65,536 mix the two inside one log p.  Held to the oracle at the
    parity bar (not to the full table's bytes: the series is its own rounding)."""
    C, slab, exp = built_long(restatement, n)
    assert sum(st.classify_wave(cvg_table(t))["series_mixed"] for t in C) >= 8
    eng = bv.BaseTypeEngine(max_sites=slab["n_sites"], min_af_value=bv.min_af(n), device=0, max_samples=1000)
    try:
        got = eng.lrt(slab)
    finally:
        eng.close()
    hold_long(got, exp)


def test_long_tables_in_tile_jobs(bv, restatement):
    """The corpus of 100,000 samples as tile jobs of width 25,000: joined rows are the row submit's records byte for byte; the
    per-site-tally finish has Fisher and SOR call sites of its own and is held to the oracle."""
    n = 100000
    C, slab, exp = built_long(restatement, n)
    for flags in (0, TILE_STATE):
        eng = bv.BaseTypeEngine(max_sites=slab["n_sites"], min_af_value=bv.min_af(n), device=0, flags=flags)
        try:
            t = eng.lrt_tiles(slab, 25000)
        finally:
            eng.close()
        hold_long(t, exp)
        if flags == 0:
            same(lrt(bv, slab)[0], t)


def test_million_sample_tables_as_rows_and_tiles(bv, restatement):
    """strand_tables.corpus_million: the family of 500,001 tables at the mode and at q ~ 1e-200, probe steps of ~4,000 tables
    and windows of ~300 rounds, the shifted family whose window starts below the live floor after a probe, 524288 x 8192
    in SOR's denominator -- as one row submit and as tile jobs of width 50,000 in both realisations."""
    n = st.MILLION
    C, slab, exp = built_long(restatement, n)
    rows, form = lrt(bv, slab)
    assert form == expected_form(n)
    hold_long(rows, exp)
    for flags in (0, TILE_STATE):
        eng = bv.BaseTypeEngine(max_sites=slab["n_sites"], min_af_value=bv.min_af(n), device=0, flags=flags)
        try:
            t = eng.lrt_tiles(slab, 50000)
        finally:
            eng.close()
        hold_long(t, exp)
        if flags == 0:
            same(rows, t)


def test_wave_tables_under_the_wave_solver_on_short_rows(bv, restatement):
    """The wave form is the short rows' form too, for shallow sites and phred-0 calls: the wave-regime, probe-span and
    round-geometry tables that fit 16,385 reads, every candidate on the one-site-per-wave solver (BV_FLAG_WAVE_SOLVER)."""
    n = 16385
    L = st.corpus_long(st.LONG_ROWS[0])
    tables = [t for name, t in zip(L.names, L) if name.startswith("wave") and sum(t) <= n]
    got = set()
    for t in tables:
        got |= st.wave_labels(t, st.classify_wave(t))
        assert st.classify(t, n, restatement.min_af(n))["candidate"], t
    assert got >= {c for c in st.required_wave_classes() if c.startswith(("wave:R=", "wave:span:", "wave:window", "wave:lane"))}
    C, slab, exp = built_long(restatement, n, tables=tables, key=(n, "wave tables"))
    base, form = lrt(bv, slab, WAVE_SOLVER)
    assert form == expected_form(n, WAVE_SOLVER)
    hold_long(base, exp)
