"""Seeded slabs whose sites are built, read count by read count, to take a chosen leaf of the LRT's allele decision tree
(test helper, not a conftest).

basevar_amd.synth.make_slab draws a REF and at most two ALT bases per site; a fourth base appears only as sequencing error,
far below min_af.  lrt() (src/basetype.cpp:130-199) branches on the number of ACTIVE bases (depth / total >= min_af) and then
on a chain of accept / reject decisions (chi2 < 24), and the number of EM runs names the leaf a site took:

    active  outcome                      n_em        active  outcome                      n_em
    1       (nothing to test)            1           3       reject at the top            1 + 3 = 4
    2       either                       1 + 2 = 3   3       one or two drops             1 + 3 + 2 = 6
    4       reject at the top            1 + 4 = 5   4       one drop                     1 + 4 + 3 = 8
    4       two or three drops           1 + 4 + 3 + 2 = 10

allele_slab() builds every leaf of LEAVES from per-base read counts (pairwise distinct: equal counts with one phred per base
are ties) and a phred RANGE per base: a "strong" base (phred >= 8) is kept, a "weak" one (phred 1..6, a tenth of the
reads or fewer) is active and then dropped by the LRT.  REF is a kept base, a dropped base, a base without reads or N, as
the leaf allows; with REF = N the four-kept leaf has four ALTs.  The widths of the phred ranges set the number of
(base, phred) bins of a site, which is what the solvers switch on (BIN_CLASSES).  mapq, rank and strand are drawn as make_slab
draws them, so the strand tables and rank sums of 2-, 3- and 4-ALT sites are compared too; ranks stay <= 100, so
synth.tag_ranks applies.

Threshold pairs put a base on the smallest depth with depth / total >= min_af, and one read below; a chi2 bracket sweeps
the read count of a phred 8..14 ALT and keeps the sites closest below and above LRT_THRESHOLD 24.  With pop-groups the group
compositions are built as well (GROUP_ROLES).  assert_leaves_hit() and assert_margins() read the ORACLE's records: a slab
that misses a leaf, or that holds a site decided by a rounding-noise margin, fails instead of passing quietly."""
import numpy as np

import basevar_amd

# one row length per kernel form and per switch between two (test_gpu_value_domain.ROWS)
ROWS = [60, 1500, 2048, 2049, 4096, 4097, 16384, 16385, 49152, 49153, 70000]
LRT_THRESHOLD = 24.0
MARGIN_REL = 1e-6  # a thousand times parity.TIE_EPS
MAX_PHRED = 93
WEAK = (1, 6)  # the phred range of a base the LRT drops

# name, active bases, kept bases, EM runs, what REF may be: a kept base, a dropped base, a base without reads ("absent"), N
LEAVES = [
    ("ref_only", 1, 1, 1, ("kept",)),
    ("nonref_only", 1, 1, 1, ("absent", "N")),
    ("nonref_depth10", 1, 1, 1, ("absent", "N")),
    ("nonref_depth11", 1, 1, 1, ("absent", "N")),
    ("two_kept", 2, 2, 3, ("kept", "N", "absent")),
    ("two_alt_dropped", 2, 1, 3, ("kept",)),
    ("two_ref_dropped", 2, 1, 3, ("dropped",)),
    ("three_reject", 3, 3, 4, ("kept", "N", "absent")),
    ("three_one_drop", 3, 2, 6, ("kept", "dropped", "N")),
    ("three_two_drops", 3, 1, 6, ("kept", "dropped", "N")),
    ("four_kept", 4, 4, 5, ("kept", "N", "kept", "kept")),
    ("four_three_kept", 4, 3, 8, ("kept", "dropped", "N")),
    ("four_two_kept", 4, 2, 10, ("kept", "dropped", "N")),
    ("four_one_kept_ref", 4, 1, 10, ("kept",)),
    ("four_one_kept_nonref", 4, 1, 10, ("dropped", "N")),
]
LEAF_NAMES = tuple(l[0] for l in LEAVES)

# class -> (fewest, most) bins of a site with four active bases; a site with m active bases holds m / 4 of that
BIN_CLASSES = {"few": (4, 16), "l8": (17, 32), "g48": (33, 48), "g128": (49, 128), "wave": (129, 4 * MAX_PHRED)}
BIN_ORDER = ("few", "l8", "g48", "g128", "wave", "q0")
# bins a four-active site of the class aims at
BIN_TARGET = {"few": 14, "l8": 28, "g48": 44, "g128": 100, "wave": 160}

# pop-group compositions, in group order; groups beyond these split the remaining members evenly
GROUP_ROLES = ("share", "alt_only", "ref_only", "empty", "small")
SMALL_GROUP = 48  # samples of the "small" group: at most 64 covered, the replay / tie hand-over


def coverage_for(n):
    return 0.5 if n <= 64 else 0.2 if n <= 4096 else 0.1 if n <= 16385 else 0.08


def class_bounds(cls, n_active, n_kept):
    """(fewest, most) bins a site of `cls` with n_active active bases, n_kept of them kept, must hold: the class's bounds
    times n_active / 4.  A dropped base holds at most WEAK's six phred values and a kept one at most phred 1..93, so the
    lower bound is capped by what the leaf can hold at all (only "wave" with one kept base of four meets the cap)."""
    lo, hi = BIN_CLASSES[cls]
    most = n_kept * MAX_PHRED + (n_active - n_kept) * (WEAK[1] - WEAK[0] + 1)
    return min(-(-lo * n_active // 4), most), hi * n_active // 4


def site_bins(slab, s):
    """Number of (base, phred) bins of site s: distinct pairs over its called cells."""
    N = int(slab["n_samples"])
    bs = np.asarray(slab["base_strand"])[s, :N]
    c = bs < 8
    return int(np.unique((bs[c] & 3).astype(np.int64) * 256 + np.asarray(slab["qual"])[s, :N][c]).size)


def _counts(T, n_active, n_kept, ref_weak_minor):
    """Pairwise distinct read counts of the active bases (kept ones first), summing to T."""
    n_weak = n_active - n_kept
    wf = 0.25 if ref_weak_minor else 0.10 if T >= 80 else 0.14
    base = [(1.0 - wf * n_weak) / n_kept] * n_kept + [wf] * n_weak
    off = (7, 3, -2, -9) if T >= 80 else (2, 1, -1, -2)
    c = [max(1, int(T * f) + off[i]) for i, f in enumerate(base)]
    c[0] += T - sum(c)
    while len(set(c)) < len(c):  # distinct counts: move single reads from a later base to the first
        for i in range(1, len(c)):
            if c.count(c[i]) > 1 and c[i] > 1:
                c[i] -= 1; c[0] += 1
                break
    assert sum(c) == T and min(c) >= 1 and len(set(c)) == len(c)
    return c


def _phreds(rng, count, lo, hi):
    """`count` phreds from lo..hi; every value of the range at least once where the count allows."""
    vals = np.arange(lo, hi + 1)
    if count >= vals.size:
        out = np.concatenate([vals, rng.integers(lo, hi + 1, count - vals.size)])
    else:
        out = rng.permutation(vals)[:count]
    return rng.permutation(out).astype(np.uint8)


def _ranges(cls, n_active, n_kept, counts):
    """Phred range per active base (kept ones first) so that the site holds about BIN_TARGET[cls] * n_active / 4 bins."""
    n_weak = n_active - n_kept
    wlo, whi = WEAK
    if cls == "few":
        whi = wlo + 2
    weak_bins = sum(min(whi - wlo + 1, c) for c in counts[n_kept:])
    target = max(n_active, BIN_TARGET[cls] * n_active // 4)
    per = max(1, (target - weak_bins) // n_kept)
    out = []
    for k in range(n_kept):
        w = min(per + (k % 2), MAX_PHRED)  # neighbouring kept bases differ in width
        hi = min(MAX_PHRED, max(40, 24 + w)) if w <= 33 else MAX_PHRED
        lo = hi - w + 1
        if lo < 8:  # only the widest ranges reach below phred 8
            lo = max(1, lo)
        out.append((lo, hi))
    out += [(wlo, whi)] * n_weak
    return out


class _Pools:
    """Which samples a read of REF / of another base may sit on, and the shares that the built pop-groups take."""

    def __init__(self, n, n_groups, rng):
        self.n, self.G = n, n_groups
        gid = np.full(n, 0xFF, np.uint8)
        order = rng.permutation(n)
        self.of = {}
        if n_groups:
            sizes = {"share": int(0.30 * n), "alt_only": int(0.10 * n), "ref_only": int(0.10 * n), "empty": max(1, int(0.05 * n)),
                     "small": min(SMALL_GROUP, max(1, n // 20))}
            at = 0
            for g, role in enumerate(GROUP_ROLES[:n_groups]):
                self.of[role] = order[at:at + sizes[role]]
                gid[self.of[role]] = g
                at += sizes[role]
            extra = n_groups - len(GROUP_ROLES)
            self.rem = []
            if extra > 0:
                each = int(0.30 * n) // extra
                for k in range(extra):
                    self.rem.append(order[at:at + each])
                    gid[self.rem[-1]] = len(GROUP_ROLES) + k
                    at += each
                # groups that would see a handful of reads per site hold reads of ONE base per site: two bases with a read
                # or two each at one phred are a tie
                self.single = each * coverage_for(n) < 40
            self.ungrouped = order[at:]
        else:
            self.rem, self.ungrouped = [], order
        self.group_id = gid

    def place(self, rng, counts_by_base, ref):
        """Sample indices per base.  Built shares: a quarter of every base's reads on the "share" group, an eighth of every
        non-REF base's reads on "alt_only", an eighth of REF's reads on "ref_only", one read in twenty on "small", none on
        "empty"; the others on the remaining samples (the evenly split groups and the samples of no group)."""
        free = {k: rng.permutation(v) for k, v in self.of.items()}
        used = {k: 0 for k in free}
        nb = len(counts_by_base)
        turn = int(rng.integers(0, 1 << 16))
        if self.rem and self.single:
            rests = [rng.permutation(np.concatenate([r for k, r in enumerate(self.rem) if (k + turn) % nb == i] + [self.ungrouped[i::nb]]))
                     for i in range(nb)]
        else:
            allrest = rng.permutation(np.concatenate(self.rem + [self.ungrouped]))
            rests = None
        at_rest = 0
        out = {}
        spare = []
        for i, (b, c) in enumerate(counts_by_base.items()):
            parts = []
            left = c
            plan = []
            if self.G:
                plan.append(("share", c // 4))
                plan.append(("ref_only" if b == ref else "alt_only", c // 8))
                plan.append(("small", c // 20))
            for role, k in plan:
                if role not in free:
                    continue
                k = min(k, left, free[role].size - used[role])
                parts.append(free[role][used[role]:used[role] + k])
                used[role] += k
                left -= k
            if rests is not None:
                assert left <= rests[i].size, "more reads than samples"
                parts.append(rests[i][:left])
                spare.append(rests[i][left:])
            else:
                assert at_rest + left <= allrest.size, "more reads than samples"
                parts.append(allrest[at_rest:at_rest + left])
                at_rest += left
            out[b] = np.concatenate(parts)
        return out, np.concatenate(spare) if rests is not None else allrest[at_rest:]


def _write_site(slab, s, rng, pools, ref, bases, counts, ranges, q0=None):
    """Writes site s: bases[i] gets counts[i] reads of phreds ranges[i]."""
    cells, unused = pools.place(rng, dict(zip(bases, counts)), ref)
    for b, c, (lo, hi) in zip(bases, counts, ranges):
        at = cells[b]
        slab["base_strand"][s, at] = b | (rng.integers(0, 2, c, dtype=np.uint8) << 2)
        slab["qual"][s, at] = _phreds(rng, c, lo, hi)
        slab["mapq"][s, at] = np.where(rng.random(c) < 0.8, 60, rng.integers(10, 60, c)).astype(np.uint8)
        slab["rpr"][s, at] = rng.integers(1, 101, c).astype(np.uint16)
    if q0 is not None:  # one phred-0 read (1 - eps == 0: the generic EM) on base q0 of `bases`
        slab["qual"][s, cells[bases[q0]][0]] = 0
    k = min(2, unused.size)  # two indel cells, as make_slab's indel_frac leaves them
    slab["base_strand"][s, unused[:k]] = 9 + np.arange(k, dtype=np.uint8)
    slab["ref_base"][s] = ref


def _leaf_site(leaf, cls, T, variant, place, rng, q0=False):
    """(ref, bases, counts, ranges, declared ALT tuple, base of the phred-0 read) of one site of `leaf`.  The phred-0 read
    makes the likelihood of the one-base subset of its own base 0 and that subset's chi2 NaN, and a NaN that comes first
    in a level's list stops the chain (std::min_element keeps it).  So that the leaf stays the declared one, the read sits
    on a kept base where two or more are kept (a NaN at the last level then stops a chain that stops there anyway), else
    on a dropped base that follows the kept one in ACGT order."""
    name, n_active, n_kept, n_em, refs = leaf
    ref_kind = refs[variant % len(refs)]
    order = [int(b) for b in rng.permutation(4)]
    in_order = sorted(order[:n_active])  # four_kept: A C G T, so REF is first, in the middle and last in ACGT order
    # which positions of the active list (ACGT order) the dropped bases hold: `place` walks them, so that a slab of six
    # classes drops the first, a middle and the last entry of the list, each with another kind of REF
    weak_at = {(place + k) % n_active for k in range(n_active - n_kept)}
    q0_at = None
    if q0:
        q0_at = 0 if n_kept >= 2 or n_active == 1 else 1
        if q0_at:
            weak_at = set(range(1, n_active))
    active = [b for i, b in enumerate(in_order) if i not in weak_at] + [b for i, b in enumerate(in_order) if i in weak_at]
    if name == "nonref_depth10":
        T = 10
    elif name == "nonref_depth11":
        T = 11
    counts = _counts(T, n_active, n_kept, name == "two_ref_dropped")
    ranges = _ranges(cls, n_active, n_kept, counts)
    if ref_kind == "kept":
        ref = active[(variant // len(refs)) % n_kept] if name != "four_kept" else (0, None, 2, 3)[variant % 4]
    elif ref_kind == "dropped":
        ref = active[n_kept + (variant // len(refs)) % (n_active - n_kept)]
    elif ref_kind == "absent":
        ref = order[n_active]
    else:
        ref = 4
    alt = tuple(sorted(b for b in active[:n_kept] if b != ref))
    return ref, active, counts, ranges, alt, q0_at


def min_active_depth(total, maf):
    """Smallest d with d / total >= maf, the comparison of basetype.cpp:137 on doubles."""
    d = max(1, int(maf * total) - 2)
    while not d / total >= maf:
        d += 1
    assert (d - 1) / total < maf
    return d


def threshold_total(n):
    if n == 16384:
        return 4096
    T = int(coverage_for(n) * n)
    return max(100, T // 100 * 100) if n <= 10000 and T >= 100 else max(T, 1)


def _empty_slab(S, n):
    pitch = (n + 15) // 16 * 16
    slab = {"n_sites": S, "n_samples": n, "pitch": pitch, "n_groups": 0,
            "base_strand": np.full((S, pitch), 8, np.uint8), "qual": np.zeros((S, pitch), np.uint8),
            "mapq": np.zeros((S, pitch), np.uint8), "rpr": np.zeros((S, pitch), np.uint16), "ref_base": np.zeros(S, np.uint8)}
    # padding cells are garbage-looking, as make_slab's: the engine must ignore everything at or beyond n_samples
    slab["base_strand"][:, n:] = 0; slab["qual"][:, n:] = 40; slab["mapq"][:, n:] = 60; slab["rpr"][:, n:] = 7
    return slab


def _clear(slab, s):
    n = int(slab["n_samples"])
    slab["base_strand"][s, :n] = 8
    for k in ("qual", "mapq", "rpr"):
        slab[k][s, :n] = 0


def oracle_records(restatement, slab):
    """(records with the restatement's n_em and chi2, group records, margins) of `slab`.  `restatement` is the fixture (the
    real reference's records where it is built) or a plain oracle.Restatement."""
    maf = basevar_amd.min_af(int(slab["n_samples"]))
    e, g, m = restatement.run_with_margins(slab, maf, n_threads=16)
    if getattr(restatement, "direct", False):  # n_em is not observable through the reference: the restatement's
        import oracle
        r, _ = oracle.Restatement().run(slab, maf, n_threads=16)
        e = e.copy()
        e["n_em"] = r["n_em"]
    return e, g, m


def allele_slab(n_samples, seed, bins, n_groups=0, restatement=None):
    """(slab, declared).  `bins`: a class of BIN_ORDER or a sequence of them (concatenated into one slab).  declared: a list
    of dicts per site -- name, n_em, alt (reference order), cls, n_active, n_kept, bins, and for pairs and brackets their
    gaps; with pop-groups also groups: {group: (n_alt, alt)} for the groups whose composition fixes the call.  With
    `restatement` (an oracle.Restatement or the fixture) the slab also holds the chi2 bracket, and every site whose oracle
    margin is below MARGIN_REL * max(1, |chi2|) is redrawn from the next sub-seed, at most eight times."""
    n = int(n_samples)
    classes = (bins,) if isinstance(bins, str) else tuple(bins)
    maf = basevar_amd.min_af(n)
    # covered depth of a site: <= 50 on rows of <= 64 samples (the per-sample replay), else 80 or more.  The depth-10 and
    # depth-11 leaves are shallow at every row length: a replayed site inside a launch of deep ones.
    T = min(50, int(coverage_for(n) * n)) if n <= 64 else max(80, int(coverage_for(n) * n))
    plan = []
    for ci, cls in enumerate(classes):
        q0 = cls == "q0"
        eff = BIN_ORDER[(seed + ci) % 5] if q0 else cls  # "q0": one of the five bin classes, by seed, plus the phred-0 read
        for li, leaf in enumerate(LEAVES):
            plan.append(dict(kind="leaf", leaf=leaf, cls=cls, eff=eff, q0=q0, variant=seed + ci + li, place=seed + ci + ci // 3))
    plan.append(dict(kind="pair", d=0)); plan.append(dict(kind="pair", d=-1))
    if restatement is not None:
        plan.append(dict(kind="bracket", side=0)); plan.append(dict(kind="bracket", side=1))
    S = len(plan)
    slab = _empty_slab(S, n)
    pools = _Pools(n, n_groups, np.random.default_rng([seed, n, 0x9001]))
    if n_groups:
        slab["n_groups"] = n_groups
        slab["group_id"] = pools.group_id
    declared = [None] * S

    def build(s, sub):
        p = plan[s]
        rng = np.random.default_rng([seed, n, s, sub])
        _clear(slab, s)
        if p["kind"] == "leaf":
            leaf = p["leaf"]
            ref, bases, counts, ranges, alt, q0_at = _leaf_site(leaf, p["eff"], T, p["variant"], p["place"], rng, p["q0"])
            _write_site(slab, s, rng, pools, ref, bases, counts, ranges, q0=q0_at)
            declared[s] = dict(name=leaf[0], n_em=leaf[3], alt=alt, cls=p["cls"], eff=p["eff"], n_active=leaf[1], n_kept=leaf[2],
                               ref=ref, bins=site_bins(slab, s))
        elif p["kind"] == "pair":
            # REF and one ALT kept, a third base of WEAK phreds on the threshold depth (active: 3 bases, 6 EM runs) or one
            # read below it (2 bases, 3 EM runs)
            tot = threshold_total(n)
            d = min_active_depth(tot, maf) + p["d"]
            order = [int(b) for b in rng.permutation(4)]
            rest = tot - d
            counts = [rest - rest // 3, rest // 3, d]
            _write_site(slab, s, rng, pools, order[0], order[:3], counts, [(25, 40), (25, 36), WEAK])
            on = p["d"] == 0
            declared[s] = dict(name="threshold_on" if on else "threshold_below", n_em=6 if on else 3, alt=(order[1],), cls=None,
                               n_active=3 if on else 2, n_kept=2, ref=order[0], bins=site_bins(slab, s), depth=d, total=tot,
                               gap=abs(d / tot - maf) / maf)

    for s in range(S):
        if plan[s]["kind"] != "bracket":
            build(s, 0)
    if restatement is not None:
        _bracket(slab, plan, declared, pools, restatement, seed, T)
        for sub in range(9):  # redraw the sites a rounding-noise margin decided, at most eight times
            e, _, m = oracle_records(restatement, slab)
            tight = [s for s in range(S) if plan[s]["kind"] != "bracket" and not _margin_ok(m[s], e["chi2"][s])]
            if not tight:
                break
            if sub == 8:
                raise RuntimeError("sites %s keep a margin below %g after eight redraws" % (tight, MARGIN_REL))
            for s in tight:
                build(s, sub + 1)
    if n_groups:
        for d in declared:
            d["groups"] = _declared_groups(d, n_groups)
    return slab, declared


def _margin_ok(margin, chi2):
    return margin >= MARGIN_REL * max(1.0, abs(float(np.nan_to_num(chi2, nan=0.0))))


def _declared_groups(d, n_groups):
    """{group: (n_alt, alt)} where the built composition fixes the call of a VARIANT site: the proportional share and the
    ALT carriers call the site's ALTs; REF carriers and the group without a covered sample call none."""
    if not d["alt"]:
        return {}
    out = {}
    for g, role in enumerate(GROUP_ROLES[:n_groups]):
        if role in ("share", "alt_only") and d["name"] in LEAF_NAMES and not d["name"].startswith("nonref_depth"):
            out[g] = (len(d["alt"]), d["alt"])
        elif role in ("ref_only", "empty"):
            out[g] = (0, ())
    return out


def _bracket(slab, plan, declared, pools, restatement, seed, T):
    """Sweeps the read count of a phred 8..14 ALT beside a strong REF; keeps the counts whose chi2 lies closest below and
    closest above LRT_THRESHOLD, among those with a margin of MARGIN_REL or more."""
    n = int(slab["n_samples"])
    maf = basevar_amd.min_af(n)
    sides = [s for s in range(len(plan)) if plan[s]["kind"] == "bracket"]
    def sweep_of(cand):
        sweep = _empty_slab(len(cand), n)
        for i, k in enumerate(cand):
            rng = np.random.default_rng([seed, n, 0xB4AC, k])
            order = [int(b) for b in rng.permutation(4)]
            _write_site(sweep, i, rng, pools, order[0], order[:2], [T - k, k], [(25, 40), (8, 14)])
        e, _, m = restatement.run_with_margins(sweep, maf, n_threads=16)[:3]
        return sweep, e["chi2"], m

    lo, hi = min_active_depth(T, maf), max(2, T // 2)
    while hi - lo > 48:  # chi2 rises with the read count: narrow the window around the crossing
        grid = sorted(set(np.linspace(lo, hi, 17).astype(int).tolist()))
        _, chi, _ = sweep_of(grid)
        up = [i for i in range(len(grid)) if chi[i] >= LRT_THRESHOLD]
        i = up[0] if up else len(grid) - 1
        if i == 0 or not up:
            break
        lo, hi = grid[i - 1], grid[i]
    cand = list(range(max(1, lo - 8), min(T - 1, hi + 8) + 1))
    sweep, chi, m = sweep_of(cand)
    ok = np.array([_margin_ok(m[i], chi[i]) for i in range(len(cand))])
    below = [i for i in range(len(cand)) if ok[i] and chi[i] < LRT_THRESHOLD]
    above = [i for i in range(len(cand)) if ok[i] and chi[i] >= LRT_THRESHOLD]
    if not below or not above:
        raise RuntimeError("the chi2 sweep of %d..%d reads of %d does not cross %g (chi2 %g..%g)" % (
            cand[0], cand[-1], T, LRT_THRESHOLD, float(np.nanmin(chi)), float(np.nanmax(chi))))
    pick = (max(below, key=lambda i: chi[i]), min(above, key=lambda i: chi[i]))
    for s, i, side in zip(sides, pick, (0, 1)):
        k = cand[i]
        order = [int(sweep["ref_base"][i])] + [b for b in range(4) if b != sweep["ref_base"][i] and (sweep["base_strand"][i, :n] & 0xB == b).any()]
        for key in ("base_strand", "qual", "mapq", "rpr"):
            slab[key][s, :n] = sweep[key][i, :n]
        slab["ref_base"][s] = sweep["ref_base"][i]
        declared[s] = dict(name="bracket_above" if side else "bracket_below", n_em=3, alt=(order[1],) if side else (), cls=None,
                           n_active=2, n_kept=1 + side, ref=order[0], bins=site_bins(slab, s), reads=k,
                           gap=abs(float(chi[i]) - LRT_THRESHOLD))


def assert_leaves_hit(declared, records, group_records=None):
    """The oracle's n_em and ALT tuple equal the declared ones at every site, every leaf name occurs, and (with group
    records) the declared (n_alt, alt) of every (site, group) holds.  Reads the records, not the builder's intent."""
    rec = getattr(records, "sites", records)
    assert len(rec) == len(declared)
    seen = set()
    for s, d in enumerate(declared):
        alt = tuple(int(a) for a in rec["alt"][s][:rec["n_alt"][s]])
        assert int(rec["n_em"][s]) == d["n_em"] and alt == d["alt"], "site %d (%s, class %s): n_em %d, ALT %s; declared %d, %s" % (
            s, d["name"], d["cls"], rec["n_em"][s], alt, d["n_em"], d["alt"])
        seen.add(d["name"])
        if d["alt"] and d["name"] in ("nonref_only", "nonref_depth11", "two_ref_dropped"):
            assert rec["qual"][s] == 5000.0, "site %d (%s): QUAL %r" % (s, d["name"], rec["qual"][s])
        if d["name"] == "nonref_depth10":
            assert rec["total_depth"][s] == 10 and rec["qual"][s] != 5000.0
        if d["name"] == "nonref_depth11":
            assert rec["total_depth"][s] == 11
        if group_records is not None and d["alt"]:
            for g, (n_alt, galt) in d.get("groups", {}).items():
                got = (int(group_records["n_alt"][s, g]), tuple(int(a) for a in group_records["alt"][s, g][:group_records["n_alt"][s, g]]))
                assert got == (n_alt, galt), "site %d (%s) group %d: %s, declared %s" % (s, d["name"], g, got, (n_alt, galt))
    miss = [x for x in LEAF_NAMES + ("threshold_on", "threshold_below") if x not in seen]
    assert not miss, "leaves %s do not occur" % miss


def assert_margins(margins, records):
    """Every site's oracle margin is MARGIN_REL * max(1, |chi2|) or more: a condition on the inputs, met by the
    reference alone."""
    rec = getattr(records, "sites", records)
    bad = [(s, float(margins[s]), float(rec["chi2"][s])) for s in range(len(rec)) if not _margin_ok(margins[s], rec["chi2"][s])]
    assert not bad, "sites decided by a rounding-noise margin (site, margin, chi2): %s" % bad[:5]


def assert_classes(declared, n_samples):
    """Every class holds the leaves with two, three and four active bases, and each of those sites holds the bins of its
    class (class_bounds).  Rows of <= 64 samples hold at most 50 reads: no class beyond their read count is asked of them."""
    if n_samples <= 64:
        return
    per = {}
    for s, d in enumerate(declared):
        if d["cls"] is None or d["n_active"] < 2:
            continue
        lo, hi = class_bounds(d["eff"], d["n_active"], d["n_kept"])
        assert lo <= d["bins"] - (1 if d["cls"] == "q0" else 0) <= hi, "site %d (%s): %d bins, class %s asks %d..%d" % (
            s, d["name"], d["bins"], d["eff"], lo, hi)
        per.setdefault(d["cls"], set()).add(d["name"])
    want = {l[0] for l in LEAVES if l[1] >= 2}
    for cls, names in per.items():
        assert names >= want, "class %s lacks %s" % (cls, sorted(want - names))
