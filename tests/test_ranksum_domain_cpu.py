"""CPU tests of the rank-sum and QUAL corpus (tests/ranksum_domain.py): every row length populates every class it can hold
-- read off the oracle's own records of the corpus slab, not off the builder's intent --, every site is a variant site
with its rank sums formed, and the oracle's three phreds are the model's (the reads ranked literally, z in float64,
math.erfc), so that the GPU tests may trust the oracle there.

Measured over the corpora of all nine row lengths (66, 88 and seven times 106 sites): the largest relative difference between
the oracle's phred and the model's is 2.78e-10 (htslib's kf_erfc against math.erfc, near the bottom of its second branch: at
|z| = 7.69, 1,480 + 20 separated reads of the 1,500-sample row, and 2.77e-10 at |z| = 7.71 on the longer rows; 6.2e-11 at most
in the first branch), below the bound of 1e-9, and no site is excluded.  Every z = 0 gives -0.0 in the oracle
(-10 * log10(1.0)), as in the model: the sign bit of each such value is asserted, in all three fields.  The test prints, per
row length, the classes populated, the targets left out as unreachable and that difference (pytest -s)."""
import math

import numpy as np
import pytest

import ranksum_domain as rd

ROWS = (60, 1500, 2048, 4096, 4097, 16385, 49152, 49153, 70000)
RTOL = 1e-9   # the bound tests/test_oracle_cpu.py uses for kf_erfc against scipy


def _z(classes):
    return {"%s:%s:%s" % (s, c, sg) for s in rd.STATS for c in classes for sg in "+-"}


# What a row length cannot hold.  |z| is at most sqrt(3 n1 n2 / (n + 1)) (complete separation; the reference's variance has no
# tie correction): 6.6 on the 30 + 29 reads of a 60-sample row, which reaches the top of the first erfc branch and nothing
# of the second, and 33.5 on 750 + 749 reads.  |z| > 37 needs about 915 + 915 reads, |z| > 38.5 about 990 + 990.
UNREACHABLE = {60: _z(("second_bottom", "mid15", "mid30", "below_cut", "above_cut", "far")),
               1500: _z(("below_cut", "above_cut", "far"))}
# QUAL is the statistic of dropping the weaker of two bases: 30 + 30 reads on phred 93 end near QUAL 2,700.
QUAL_UNREACHABLE = {60: {"qual:2900-3076", "qual:3077-3130", "qual:zero", "qual:zero_neighbour"}}


def test_model_on_sites_ranked_by_hand():
    # 3 2 2 1 descending, REF holds 3 and 1: ranks 1 and 4, the tie 2.5 each
    assert rd.two_R([3, 1], [2, 2]) == 10 and rd.z_of(10, 2, 2) == 0.0
    # 5 5 | 1: the REF reads share ranks 1 and 2
    assert rd.two_R([5, 5], [1]) == 6
    assert abs(rd.z_of(6, 2, 1) + 1.0 / math.sqrt(2 * 1 * 4 / 12.0)) < 1e-15
    assert rd.two_R([], [4, 4]) == 0 and rd.z_of(0, 0, 2) is None and rd.phred_of_z(None) == 10000.0
    assert math.copysign(1.0, rd.phred_of_z(0.0)) == -1.0 and rd.phred_of_z(0.0) == 0.0
    assert rd.phred_of_z(37.0000001) == 10000.0 and 2970 < rd.phred_of_z(36.9) < 2990
    # the closed form of the two-value family is the literal ranking's z
    for n1, n2, target in ((1000, 999, 36.99), (30, 29, -6.8), (69875, 125, -3.0), (7, 400, 2.0)):
        r_hi, a_hi, z = rd.nearest_two_value(n1, n2, target)
        ref, alt = rd.two_value_reads(n1, n2, r_hi, a_hi, 255, 256)
        assert abs(rd.z_of(rd.two_R(ref, alt), n1, n2) - z) <= 1e-12 * max(1.0, abs(z))
    assert [rd.regime(z) for z in (None, 0.0, -7.0, 7.1, -37.0, 37.1)] == ["no_z", "z0", "first", "second", "second", "cut"]
    assert [rd.z_class(z) for z in (0.0, 0.5, -7.07, 7.08, 15.0, -30.0, 36.99, -37.01, 38.0, 39.0)] == [
        "z0", "small", "first_top", "second_bottom", "mid15", "mid30", "below_cut", "above_cut", None, "far"]


@pytest.mark.parametrize("n", ROWS)
def test_corpus_populates_its_classes_and_the_oracle_is_the_model(restatement, n):
    C = rd.corpus(n)
    Q, excluded = rd.qual_sites(restatement, n)
    sites = list(C) + Q
    maf = restatement.min_af(n)
    assert C.min_af == maf and len(set(C.names)) == len(C) and len(sites) <= 125
    exp, _ = restatement.run(rd.slab(sites, n), maf, n_threads=8)
    got, worst, closest = set(), (0.0, None), {-1: None, 1: None}
    for site, rec in zip(sites, exp):
        assert (int(rec["status"]) & 0x12) == 0x12, "%s: not a variant site with rank sums (status 0x%x)" % (site["name"], rec["status"])
        assert int(rec["depth"][0]) == site["n1"] and int(rec["depth"][1]) == site["n2"] and int(rec["total_depth"]) == site["n1"] + site["n2"]
        assert int(rec["n_alt"]) == 1 and int(rec["alt"][0]) == 1, site["name"]
        z = rd.site_z(site)
        for s, want in zip(rd.STATS, rd.model(site)):
            assert rd.clear_of_boundaries(z[s]), (site["name"], s, z[s])
            have = float(rec[rd.FIELD[s]])
            if want == 10000.0 or want == 0.0:
                # 10000 and the zeros exactly; a zero is -0.0 in the oracle as in the model
                assert have == want and np.signbit(have) == np.signbit(want), (site["name"], s, have, want)
                assert want == 10000.0 or np.signbit(have), (site["name"], s)
            else:
                rel = abs(have - want) / abs(want)
                if rel > worst[0]:
                    worst = (rel, "%s %s |z| = %.6g" % (site["name"], s, abs(z[s])))
                assert rel <= RTOL, (site["name"], s, have, want, rel)
            if z[s] is not None and abs(z[s]) > 30:
                side = 1 if abs(z[s]) > rd.CUT else -1
                if closest[side] is None or abs(abs(z[s]) - rd.CUT) < closest[side]:
                    closest[side] = abs(abs(z[s]) - rd.CUT)
        got |= rd.labels(site, rec)
    required = rd.required_classes(n) | rd.required_qual_classes()
    print("%d samples, %d sites: %d classes populated; not reachable: %s" % (n, len(sites), len(required & got), sorted(required - got)))
    for line in list(C.unreachable) + excluded:
        print("   left out: " + line)
    print("   largest relative difference oracle / model: %.2e at %s" % worst)
    assert required - got == UNREACHABLE.get(n, set()) | QUAL_UNREACHABLE.get(n, set())
    assert bool(UNREACHABLE.get(n)) <= bool(C.unreachable) and bool(QUAL_UNREACHABLE.get(n)) <= bool(excluded)
    if n >= 2048:
        # the cut at 37 from both sides: the nearest site below and the nearest above are within 0.1 of it
        assert closest[-1] < 0.1 and closest[1] < 0.1, closest
        assert any("fewer than 34 bits" in line for line in excluded)
    # the QUAL sites keep their margins: a class counts only MARGIN inside its range (labels), a 10000 is an exact zero of p
    for site, rec in zip(sites, exp):
        if site.get("kind") == "qual":
            q = float(rec["qual"])
            assert q == 10000.0 or q < rd.QUAL_FLOOR * (1 - 1e-4), (site["name"], q)


def test_ranks_up_to_8191_for_the_tagged_layout(restatement):
    n = 2048
    C = rd.corpus(n, 8191)
    assert max(int(s[k]["rpr"].max()) for s in C for k in ("ref", "alt") if s[k]["rpr"].size) == 8191
    exp, _ = restatement.run(rd.slab(C, n), restatement.min_af(n), n_threads=8)
    got = set()
    for site, rec in zip(C, exp):
        got |= rd.labels(site, rec)
    assert rd.required_classes(n, 8191) - got == set()


@pytest.mark.parametrize("n", [60, 1500, 16385, 70000])
def test_orders_put_every_pair_of_regimes_on_adjacent_sites(n):
    C = rd.corpus(n)
    orders, pairs, wanted = rd.orders(C)
    assert len(orders) == 3 and all(sorted(o.tolist()) == list(range(len(C))) for o in orders)
    assert np.array_equal(orders[0], np.arange(len(C))) and np.array_equal(orders[1], np.arange(len(C))[::-1])
    assert pairs >= wanted
    regimes = {s: {a for (t, a, b) in wanted if t == s} for s in rd.STATS}
    for s in rd.STATS:
        assert regimes[s] == (set(rd.REGIMES) if n > 2000 else set(rd.REGIMES) - {"cut"} - ({"second"} if n == 60 else set())), (s, regimes[s])


def test_slab_moves_a_site_with_its_order():
    C = rd.corpus(1500)[:12]
    order = np.random.default_rng(3).permutation(len(C))
    a, b = rd.slab(C, 1500), rd.slab(C, 1500, order)
    assert a["pitch"] == 1504 and (a["base_strand"][:, 1500:] == 0).all()
    for k in ("base_strand", "qual", "mapq", "rpr"):
        assert np.array_equal(a[k][order], b[k])
    # both strands on REF and on ALT, the reads spread over the row
    bs = a["base_strand"][0, :1500]
    assert {0, 1, 4, 5} <= set(np.unique(bs).tolist()) and np.flatnonzero(bs < 8).max() > 1400
