"""CPU tests of the strand-table corpus (tests/strand_tables.py): every row length populates every class of table it can
hold -- read off the oracle's own cvg_sb / var_sb of the corpus slab, not off the builder's intent --, and the oracle's
Fisher test is the exact two-sided rule on every one of these tables, so that the GPU tests may trust it there."""
import decimal
import math

import numpy as np
import pytest

import strand_tables as st

ROWS = (1500, 2048, 4096, 4097, 16385, 49152, 49153)

# What a row length cannot hold.  min_af is 0.01 up to 10,000 samples: a hom-ref site keeps its ALT reads below 1 % of
# the row, so 21 ALT reads (R = 22) need more than 2,100 reads and 31 or 32 (R = 32, 33) more than 3,100.  R ~ 1,000 takes
# 1,998 reads.  A steep end -- the family's first table below e^-760 beside an ordinary q -- has ln p ~ -ln C(n, R - 1):
# with every read of the row that is -556 and -642 at R = 256 on 1,500 and 2,048 reads (-827 on 4,096), and at R = 129
# it is -649 on 16,385 reads (-790 on 49,152).
_STEEP = {"steep_end:R=%d:%s" % (R, e) for R in st.STEEP_R for e in ("imin", "imax")}
_STEEP_129 = {c for c in _STEEP if "R=129" in c}
UNREACHABLE = {
    1500: {"lane:R=22", "lane:R=31", "lane:R=32", "homref:R=33:g16", "probed:R~1000"} | _STEEP,
    2048: {"lane:R=22", "lane:R=31", "lane:R=32", "homref:R=33:g16"} | _STEEP,
    4096: _STEEP_129, 4097: _STEEP_129, 16385: _STEEP_129, 49152: set(), 49153: set(),
}


def cvg_table(t):
    t = tuple(t) + (0, 0)
    return (t[0], t[1], t[2] + t[4], t[3] + t[5])


def test_classify_on_tables_of_known_routing():
    maf = st.min_af(10000)
    assert maf == float(np.float32(0.01))
    c = st.classify((500, 480, 6, 6), 10000, maf)           # 12 ALT reads of 992: a candidate, product form
    assert (c["regime"], c["R"], c["m"], c["candidate"], c["solver"]) == ("product", 13, 12, True, "g16")
    c = st.classify((500, 480, 7, 6), 10000, maf)
    assert (c["regime"], c["R"], c["m"]) == ("narrow", 14, 13)
    c = st.classify((5000, 4800, 7, 6), 10000, maf)         # 13 of 9,813: hom-ref, 14 tables, one lane
    assert (c["regime"], c["candidate"], c["solver"], c["position"]) == ("lane", False, "lane", "interior")
    c = st.classify((5000, 4800, 7, 6), 10000, maf, phred0=True)
    assert (c["regime"], c["candidate"], c["solver"]) == ("narrow", True, "wave")
    c = st.classify((5000, 4800, 20, 12), 10000, maf)       # hom-ref, 33 tables: the 16-lane solver
    assert (c["regime"], c["R"], c["candidate"], c["hom_ref"]) == ("narrow", 33, True, True)
    c = st.classify((64, 0, 0, 64), 10000, maf)
    assert (c["regime"], c["R"], c["position"], c["solver"]) == ("narrow", 65, "imax", "g16")
    c = st.classify((64, 64, 64, 65), 10000, maf)
    assert (c["regime"], c["R"], c["imin"], c["imax"]) == ("probed", 129, 0, 128)
    c = st.classify((20, 12, 3, 29), 10000, maf)            # 64 reads: replayed by the wave solver
    assert (c["regime"], c["solver"]) == ("narrow", "wave")
    c = st.classify((0, 0, 50, 50), 10000, maf)
    assert (c["regime"], c["candidate"]) == ("degenerate", True)
    c = st.classify((500, 480, 6, 6), 60000, st.min_af(60000))
    assert c["solver"] == "wave"
    assert abs(st.classify((505, 0, 0, 505), 1500, maf)["log10q"] + 302.4) < 0.05
    assert st.classify((560, 0, 0, 560), 1500, maf)["log10q"] < st.ZERO_LOG10


@pytest.mark.parametrize("n", ROWS)
def test_corpus_reaches_every_class_the_row_length_holds(restatement, n):
    C = st.corpus(n)
    maf = restatement.min_af(n)
    assert C.min_af == maf
    assert len(C) == len(C.names) == len(set(C)) and len(C) <= 125
    assert all(sum(t) <= n for t in C)
    slab = st.slab(C, n)
    exp, _ = restatement.run(slab, maf, n_threads=8)
    for t, rec in zip(C, exp):
        assert tuple(rec["cvg_sb"]) == cvg_table(t)
    got = st.site_classes(exp, n, maf)
    required = st.required_classes(n)
    print("%d samples, %d tables: %d classes populated; not reachable: %s" % (n, len(C), len(required & got), sorted(required - got)))
    for line in C.unreachable:
        print("   left out: " + line)
    assert required - got == UNREACHABLE[n]
    # a class that is declared out of reach has its left-out targets named by the builder
    assert bool(UNREACHABLE[n]) <= bool(C.unreachable)


@pytest.mark.parametrize("n", ROWS)
def test_the_oracle_is_the_exact_rule_on_every_corpus_table(restatement, n):
    """restatement.fisher against the two-sided rule over an exact hypergeometric pmf in 60-digit arithmetic: 1e-9
    relative from 2^-1040 up, exactly 0 where q underflows, and no table in between (there a double keeps too few bits
    for the reference's own sum to be defined to 1e-6).  The helper's serial walk (which chose the deep-tail tables) agrees with the oracle's to 5e-10."""
    D = decimal.Decimal
    floor = D(2) ** -1040
    worst = (D(0), None)
    tables = set(cvg_table(t) for t in st.corpus(n))
    assert any(st.log10_q(t) < st.ZERO_LOG10 for t in tables) and any(0.0 < restatement.fisher(*t) < 2.0 ** -1022 for t in tables)
    for t in sorted(tables):
        p = restatement.fisher(*t)
        w = st.serial_walk(t)   # (CPython's lgamma is its own, not the C library's: not to the bit)
        assert (p == 0.0) == (w == 0.0) and abs(p - w) <= 5e-10 * p, (t, p, w)
        if st.log10_q(t) < st.ZERO_LOG10:
            assert p == 0.0, t
            continue
        assert p >= 2.0 ** -1040, (t, p)            # the underflow-band condition: no oracle p in (0, 2^-1040)
        e = st.exact_two_sided(t)
        assert e >= floor
        rel = abs(D(p) - e) / e
        if rel > worst[0]:
            worst = (rel, t)
        assert rel <= D("1e-9"), (t, p, float(e), float(rel))
    print("%d samples: largest relative error of the oracle %.2e at %s" % (n, worst[0], worst[1]))


def test_orders_put_every_regime_into_every_group_slot():
    for n in (1500, 16385):
        C = st.corpus(n)
        orders, slots, pairs = st.wave_orders(C, n, C.min_af)
        assert len(orders) == 4 and all(sorted(o.tolist()) == list(range(len(C))) for o in orders)
        assert slots >= {(k, s) for k in st.WAVE_KINDS for s in range(4)}
        assert pairs >= {(a, b) for a in st.WAVE_KINDS for b in st.WAVE_KINDS}


def test_slab_moves_a_site_with_its_order():
    C = st.corpus(1500)[:12]
    order = np.random.default_rng(3).permutation(len(C))
    a, b = st.slab(C, 1500), st.slab(C, 1500, order)
    assert a["pitch"] == 1504 and (a["base_strand"][:, 1500:] == 0).all()
    for k in ("base_strand", "qual", "mapq", "rpr"):
        assert np.array_equal(a[k][order], b[k])


# ------------------------------------------------------------------------------------------------ long rows: the wave form
# What a long row cannot hold.  A product of two cells that wraps to 0 needs 131,072 reads and 65537 x 65535 two more
# beside 2,000 others: 140,000 samples hold them, 100,000 do not.  The shifted family whose window starts below the live
# floor after a probe needs one probe step (span // 63 + 1 tables) to span ~600 nats, i.e. ~15 sigma of the family: a step is
# 4.5 sigma at 100,000 reads and 5.4 at 140,000 (15.6 at 1,000,000: corpus_million has the class).  At 140,000 reads the
# reference's own walk is 5e-10 to 6e-10 off the exact rule on each of the sixteen q ~ 1e-300 tables corpus() tries, so
# its rule (5e-10) keeps them out.
_WRAPS = {"sor:den=65537x65535", "sor:den=65537x65537", "sor:wrap0:both", "sor:wrap0:den", "sor:wrap0:num"}
UNREACHABLE_LONG = {
    100000: (set(), _WRAPS | {"wave:shifted_below_floor_after_probe"}),
    140000: ({"probed:q300:left", "probed:q300:right"}, {"wave:shifted_below_floor_after_probe"}),
}
_long = {}


def long_records(n):
    """(corpus, slab, the restatement's own records) of a long corpus, computed once per session."""
    if n not in _long:
        import oracle
        C = st.corpus_million() if n == st.MILLION else st.corpus_long(n)
        slab = st.slab(C, n)
        _long[n] = (C, slab, oracle.Restatement().run(slab, C.min_af, n_threads=8)[0])
    return _long[n]


def test_classify_wave_on_tables_of_known_routing():
    w = st.classify_wave((500, 480, 6, 6))                  # a row margin of 12: product form, whatever R
    assert (w["regime"], w["R"], w["m"]) == ("product", 13, 12)
    w = st.classify_wave((300, 1, 280, 0))                  # a column margin of 1: two tables, no small row margin
    assert (w["regime"], w["R"], w["lane"]) == ("lanes", 2, 0)
    w = st.classify_wave((400, 394, 32, 31))                # 63 ALT reads: imin = 400 - 31, 64 tables, the observed one on lane 31
    assert (w["regime"], w["R"], w["imin"], w["lane"], w["rounds"]) == ("lanes", 64, 369, 31, 1)
    w = st.classify_wave((400, 394, 32, 32))                # 65 tables: two rounds over the whole family, no probes
    assert (w["regime"], w["R"], w["window"], w["rounds"], w["lane"], w["same_round"]) == ("rounds", 65, (368, 432), 2, 32, True)
    assert "steps" not in w and not w["shifted"] and not w["below_floor"] and not w["q0"]
    w = st.classify_wave((400, 394, 128, 127))              # 256 tables: four whole rounds, the last table on lane 63
    assert (w["regime"], w["window"], w["rounds"]) == ("rounds", (273, 528), 4)
    w = st.classify_wave((400, 394, 128, 128))              # 257: probed, spans 128 | 128 -> steps 3 | 3
    assert (w["regime"], w["steps"]) == ("probed", (3, 3))
    # probes at 272 + 3 g and 528 - 3 g: the window ends at probe points, and no further from the observed table than the
    # points where ln p falls below ln q - 60 (sigma of this family is ~7 tables: 11 sigma ~ 77 tables, + one step)
    wl, wr = w["probe_window"]
    assert (wl - 272) % 3 == 0 and (528 - wr) % 3 == 0 and 272 < wl < 400 - 70 and 400 + 70 < wr < 528
    assert st.log_p((400, 394, 128, 128), wl) < st.log_p((400, 394, 128, 128), 400) - 60 <= st.log_p((400, 394, 128, 128), wl + 3)
    for span, step in ((62, 1), (63, 2), (64, 2), (125, 2), (126, 3)):
        assert st.classify_wave((span, 999 - span, 999 - span, 14000))["steps"][0] == step
    w = st.classify_wave((600, 0, 0, 600))                  # q = C(1200, 600)^-1 ~ e^-828: exp() is 0, no walk
    assert (w["regime"], w["q0"]) == ("probed", True) and "window" not in w
    w = st.classify_wave((0, 0, 50, 50))
    assert w["regime"] == "degenerate"
    # (k, 0, 0, k) k = 520: ln q = -ln C(1040, 520) = -(1040 ln 2 - ln(520 pi) / 2) = -717.17: live but shifted; the symmetric family's two ends are the only
    # tables of at least q, L* = imin and R* = imax: 17 rounds apart
    w = st.classify_wave((520, 0, 0, 520))
    assert (w["shifted"], w["q0"], w["lstar"], w["rstar"], w["same_round"]) == (True, False, 0, 520, False)
    assert abs(st.log_p((520, 0, 0, 520), 520) + 717.17) < 0.01
    # log-factorial arguments: the cells 3 | 46341 | 46341 | 5 stay below 65,536 but the margin n = 92,690 does not
    w = st.classify_wave((3, 46341, 46341, 5))
    assert w["series"] and not w["series_mixed"]
    w = st.classify_wave((2850, 150, 92150, 4850))          # one cell beyond 65,536, three below
    assert w["series"] and w["series_mixed"] and w["R"] == 3001 and not w["below_floor"]
    w = st.classify_wave((300, 280, 40, 20))
    assert not w["series"]
    # the observed table's lane counts from the window's first table: (64, 63, 363, 364) is table 64 of the family 0..127
    w = st.classify_wave((64, 63, 363, 364))
    assert (w["regime"], w["R"], w["lane"], w["rounds"]) == ("rounds", 128, 0, 2)
    w = st.classify_wave((63, 65, 365, 363))
    assert (w["R"], w["lane"], w["rounds"]) == (129, 63, 3)


def test_the_million_sample_list_holds_its_classes():
    """The shifted family whose window starts below the live floor after a probe, populated: one probe step of the R = 500,001
    family is 3,847 tables (15.4 sigma), from ln p = -1,060 to above ln q - 60."""
    C = st.corpus_million()
    assert len(C) <= 12 and not C.unreachable and all(sum(t) <= st.MILLION for t in C)
    got = set()
    for t in C:
        got |= st.wave_labels(t, st.classify_wave(t))
    print("1,000,000 samples, %d tables: %s" % (len(C), sorted(got)))
    assert {"wave:shifted_below_floor_after_probe", "wave:rounds>=100", "wave:LR:far_apart", "wave:LR:same_round",
            "wave:steep:R=20001", "wave:series_mixed", "sor:wrap0:den"} <= got
    t = C[C.names.index("million shifted, first table below the live floor after a probe, left of the mode")]
    w = st.classify_wave(t)
    assert w["shifted"] and w["below_floor"] and w["steps"][0] > 3000 and w["window"][0] > w["probe_window"][0]
    assert st.log_p(t, w["probe_window"][0]) + st.SHIFT < st.LIVE_FLOOR <= st.log_p(t, w["window"][0]) + st.SHIFT
    assert st.log_p(t, w["window"][0] - 1) + st.SHIFT < st.LIVE_FLOOR
    assert any(t == (k, 0, 0, k) for t in C for k in (500000,)) and (1000, 524288, 8192, 1000) in C


@pytest.mark.parametrize("n", st.LONG_ROWS)
def test_long_corpus_reaches_every_class_the_row_length_holds(n):
    """corpus_long(n): every class of corpus(n) and every wave-form class, read off the oracle's own cvg_sb / var_sb."""
    C, slab, exp = long_records(n)
    maf = C.min_af
    assert len(C) == len(C.names) == len(set(C)) and len(C) <= 160
    assert all(sum(t) <= n for t in C)
    for t, rec in zip(C, exp):
        assert tuple(rec["cvg_sb"]) == cvg_table(t)
    base, wave = UNREACHABLE_LONG[n]
    got = st.site_classes(exp, n, maf)
    required = st.required_classes(n)
    wgot = st.wave_site_classes(exp)
    wreq = st.required_wave_classes()
    print("%d samples, %d tables: %d + %d classes populated; not reachable: %s" % (
        n, len(C), len(required & got), len(wreq & wgot), sorted((required - got) | (wreq - wgot))))
    for line in C.unreachable:
        print("   left out: " + line)
    assert required - got == base
    assert wreq - wgot == wave
    # every class that is out of reach has its left-out targets named by the builder
    text = "\n".join(C.unreachable)
    assert ("q300" in text) == bool(base)
    assert "shifted, first table below the live floor after a probe" in text
    assert ("wraps to 0" in text and "65537 x 65535" in text and "65537 x 65537" in text) == bool(wave & _WRAPS)
    # BV_SITE_SOR_OVERFLOW of the oracle: a product of either table above 2^31 - 1, and only then
    for t, rec in zip(C, exp):
        want = st.overflows(tuple(int(x) for x in rec["cvg_sb"])) or (rec["n_alt"] > 0 and st.overflows(tuple(int(x) for x in rec["var_sb"])))
        assert bool(rec["status"] & 0x20) == bool(want), t
    assert (exp["status"] & 0x20).any() and not (exp["status"] & 0x20).all()


@pytest.mark.parametrize("n", st.LONG_ROWS)
def test_the_oracle_is_the_exact_rule_on_every_long_corpus_table(restatement, n):
    """As test_the_oracle_is_the_exact_rule_on_every_corpus_table, on the long corpora: 1e-9 relative from 2^-1040 up, exactly 0
    where q underflows, and no table in between."""
    D = decimal.Decimal
    worst = (D(0), None)
    tables = set(cvg_table(t) for t in st.corpus_long(n))
    for t in sorted(tables):
        p = restatement.fisher(*t)
        if st.log10_q(t) < st.ZERO_LOG10:
            assert p == 0.0, t
            continue
        assert p >= 2.0 ** -1040, (t, p)
        e = st.exact_two_sided(t)
        rel = abs(D(p) - e) / e
        if rel > worst[0]:
            worst = (rel, t)
        assert rel <= D("1e-9"), (t, p, float(e), float(rel))
    print("%d samples: largest relative error of the oracle %.2e at %s" % (n, worst[0], worst[1]))


def test_the_oracle_is_the_compiled_reference_at_a_million_samples(reference):
    """The exact rule is too slow at 1,000,000 reads: there the restatement is held to the compiled reference, bit for bit on
    FS and SOR and on BV_SITE_SOR_OVERFLOW."""
    C, slab, exp = long_records(st.MILLION)
    ref = reference.run(slab, C.min_af, n_threads=8)[0]
    for f in ("cvg_sb", "var_sb", "n_alt", "cvg_fs", "cvg_sor", "var_fs", "var_sor"):
        assert np.array_equal(exp[f], ref[f], equal_nan=True), f
    assert np.array_equal(exp["status"] & 0x20, ref["status"] & 0x20)
    i = C.index((1000, 524288, 8192, 1000))                 # 524288 x 8192 = 2^32: the denominator wraps to 0
    assert exp["cvg_sor"][i] == 10000.0 and exp["status"][i] & 0x20
    assert ((exp["cvg_fs"] > 1900) & (exp["cvg_fs"] < 2200)).sum() >= 4     # the q ~ 1e-200 tables: p is no 0


@pytest.mark.parametrize("n", st.LONG_ROWS)
def test_restatement_is_the_compiled_reference_on_the_sor_products(reference, n):
    """FS, SOR and BV_SITE_SOR_OVERFLOW of oracle/refcpu.c against the reference as compiled, on every table of the long
    corpora -- the SOR-product tables among them: a product of two cells just below and just above 2^31 in the numerator and
    in the denominator, one that wraps to -1, to a small positive number and to exactly 0 (where the guard of
    basetype.cpp:286 as compiled gives 10000 and no division by 0)."""
    C, slab, exp = long_records(n)
    ref = reference.run(slab, C.min_af, n_threads=8)[0]
    sor = [i for i, name in enumerate(C.names) if name.startswith("SOR") and " x " in name]
    assert len(sor) == (10 if n >= 133074 else 5)
    for f in ("cvg_sb", "var_sb", "n_alt", "cvg_fs", "cvg_sor", "var_fs", "var_sor"):
        assert np.array_equal(exp[f], ref[f], equal_nan=True), (f, [C.names[i] for i in np.nonzero(exp[f] != ref[f])[0][:4]])
    assert np.array_equal(exp["status"] & 0x20, ref["status"] & 0x20)
    assert np.isfinite(exp["cvg_sor"]).all() and np.isfinite(exp["var_sor"][exp["n_alt"] > 0]).all()
    by_name = {C.names[i]: exp[i] for i in sor}
    r = by_name["SOR den 46340 x 46341: below 2^31, no flag"]
    assert not r["status"] & 0x20 and r["cvg_sor"] == 15 / (46340 * 46341)
    r = by_name["SOR den 46341 x 46341: wraps negative"]
    assert r["status"] & 0x20 and r["cvg_sor"] == 15 / (46341 * 46341 - 2 ** 32)
    r = by_name["SOR num 46341 x 46341: wraps negative"]
    assert r["status"] & 0x20 and r["cvg_sor"] == (46341 * 46341 - 2 ** 32) / 99
    r = by_name["SOR: the CVG table overflows (46341 x 46341), the VCF table does not (46341 x 46340)"]
    assert r["status"] & 0x20 and r["cvg_sor"] < 0 < r["var_sor"]
    if n >= 133074:
        assert by_name["SOR den 65536 x 65536: wraps to 0"]["cvg_sor"] == 10000.0
        assert by_name["SOR den 65536 x 65536 wraps to 0 over a numerator of 0"]["cvg_sor"] == 10000.0
        assert by_name["SOR num 65536 x 65536: wraps to 0"]["cvg_sor"] == 0.0
        assert by_name["SOR den 65537 x 65535: wraps to -1"]["cvg_sor"] == -1e6
        assert by_name["SOR den 65537 x 65537: wraps to 131073"]["cvg_sor"] == 1e6 / 131073
        assert all(by_name[k]["status"] & 0x20 for k in by_name if "6553" in k)
