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
