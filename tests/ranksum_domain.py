"""Sites built at a chosen z of the three Wilcoxon rank sums, and at a chosen QUAL (a test helper, not a conftest).

MQRankSum, ReadPosRankSum and BaseQRankSum are -10 log10 of a two-sided normal tail of z, with z from the rank sum of the
REF reads among the REF and ALT reads (src/algorithm.h:76-136).  Slabs that draw mapq, rank and phred independently of the
read's class keep |z| near 1.  Here a site is built from a target: a statistic (mq, rpr, bq), a z, and where its values
sit in the value range; the two statistics not under test are constant on every read (all ties, z = 0).

  corpus()      the sites of one row length, with the targets that row length cannot hold named in `unreachable`;
  qual_sites()  two-base sites whose ALT read count is swept against the oracle's chi2 into named QUAL ranges;
  slab()        one site per entry, REF A, one ALT base C on both strands, in a given order of the sites;
  model()       the expected (mq, rpr, bq) phreds: the reads ranked literally -- sorted descending, ties on their average
                rank --, 2R in Python integers, z in float64 by the formula of algorithm.h:130-132, p = math.erfc(|z| / sqrt 2),
                -10 log10 p, or 10000 where n_ref = 0, n_alt = 0 or |z| > 37 (kf_erfc returns 0 there).  It shares no code with
                the oracle or with the kernels' histogram formula;
  labels()      the classes a site populates, read off an oracle record and the model's z; required_classes() what a row
                length is asked to populate;
  orders()      the identity order, the reversed one and a seeded permutation of the sites.

The simplest family has two values lo < hi: r_hi of n1 REF reads and a_hi of n2 ALT reads hold hi, and
z = (n1 a_hi - n2 r_hi) / (2 sqrt(n1 n2 (n + 1) / 12)) (no tie correction in the reference), so an integer search finds
the point nearest a target; n2 = n1 - 1 makes every integer a numerator.  |z| is at most sqrt(3 n1 n2 / (n + 1)):
6.6 on the 59 reads of a 60-sample row, 33.5 on 1,499 reads; |z| > 37 needs about 915 + 915 reads.

orders() is a MODEL of the finish that forms the mq and rpr phreds of up to 64 sites at once, one site per lane
(bv_pass2.hip, bv_fused_stream.h), not a record of what ran: every site of the corpus is a variant site, so neighbours in
site order are taken to sit in neighbouring lanes, and the three orders between them put every ordered pair of the
regimes z0, first erfc branch, second branch, above the cut and no z (n1 == 0) of each statistic onto adjacent sites.
Which lanes two sites really share is the kernels' business; every order is held to the oracle whatever they met."""
import functools
import math

import numpy as np

STATS = ("mq", "rpr", "bq")
FIELD = {"mq": "mq_ranksum", "rpr": "rpr_ranksum", "bq": "bq_ranksum"}
PLANE = {"mq": "mapq", "rpr": "rpr", "bq": "qual"}
CONST = {"mq": 60, "rpr": 7, "bq": 30}   # the value of a statistic that is not under test
CUT = 37.0                               # kf_erfc: z > 37 gives p = 0
BRANCH = 10.0 / math.sqrt(2.0)           # kf_erfc: the rational form below, the continued fraction from here on
MARGIN = 1e-6                            # relative distance every |z| keeps from CUT and BRANCH
# |z| classes: name -> (lo, hi), lo <= |z| < hi unless said otherwise in z_class()
Z_CLASSES = {"small": (0.0, 1.0), "first_top": (6.5, BRANCH), "second_bottom": (BRANCH, 7.6), "mid15": (14.0, 16.0),
             "mid30": (29.0, 31.0), "below_cut": (36.5, CUT), "above_cut": (CUT, 37.5), "far": (38.5, math.inf)}
Z_TARGET = {"small": 0.5, "first_top": 6.8, "second_bottom": 7.3, "mid15": 15.0, "mid30": 30.0, "below_cut": 36.99,
            "above_cut": 37.01, "far": 1e9}
REGIMES = ("z0", "first", "second", "cut", "no_z")
# (lo, hi) pairs the sites of a statistic cycle through; the layout classes below name some of them
PAIRS = {"mq": [(20, 50), (5, 250), (63, 64), (127, 128), (191, 192), (0, 255)],
         "rpr": [(3, 40), (255, 256), (1023, 1024), (7, 60000), (7, 8191), (0, 65535), (2047, 2048)],
         "bq": [(20, 35), (15, 16), (63, 64), (30, 93), (10, 41)]}
EDGE_PAIRS = {"mq": [(63, 64), (127, 128), (191, 192)], "rpr": [(255, 256), (1023, 1024), (7, 60000), (7, 8191)],
              "bq": [(15, 16), (63, 64)]}
LOW_ALT_PHRED = 6      # the ALT reads of the "REF on phred 41" site: the LRT still calls them
QUAL_CLASSES = {"qual:60-120": (60.0, 120.0), "qual:~1000": (950.0, 1050.0), "qual:2900-3076": (2900.0, 3076.0),
                "qual:3077-3130": (3077.0, 3130.0)}
QUAL_FLOOR = 10.0 * 1040 * math.log10(2.0)   # 3130.7: beyond, p < 2^-1040 keeps fewer than 34 bits (strand_tables.P_FLOOR_LOG10)


def min_af(n_samples, user_min_af=0.01):
    """(double)std::min(float(100) / n, min_af) of the caller, in float arithmetic."""
    return float(min(np.float32(100.0) / np.float32(n_samples), np.float32(user_min_af)))


# ------------------------------------------------------------------------------------------------ the model
def two_R(ref_vals, alt_vals):
    """Twice the rank sum of the REF reads, a Python integer: all reads sorted descending, a block of equal values on
    positions i..j (from 1) gives each of its reads the rank (i + j) / 2."""
    v = np.concatenate([np.asarray(ref_vals, np.int64), np.asarray(alt_vals, np.int64)])
    is_ref = np.zeros(v.size, np.int64)
    is_ref[:len(ref_vals)] = 1
    o = np.argsort(-v, kind="stable")
    sv, sr = v[o], is_ref[o]
    first = np.flatnonzero(np.concatenate([[True], sv[1:] != sv[:-1]]))
    last = np.concatenate([first[1:], [v.size]])   # one past the block, from 0: the block's last position from 1
    refs = np.add.reduceat(sr, first)
    return sum(int(c) * (int(i) + 1 + int(j)) for c, i, j in zip(refs, first, last) if c)


def z_of(twoR, n1, n2):
    """algorithm.h:130-132 in float64; None without a REF or an ALT read."""
    if n1 == 0 or n2 == 0:
        return None
    r1 = float(twoR) / 2.0
    e = float(n1 * (n1 + n2 + 1)) / 2.0
    return (r1 - e) / math.sqrt(float(n1 * n2 * (n1 + n2 + 1)) / 12.0)


def phred_of_z(z):
    if z is None or abs(z) > CUT:
        return 10000.0
    return -10.0 * math.log10(math.erfc(abs(z) / math.sqrt(2.0)))


def site_z(site):
    """{statistic: z or None} of a site."""
    n1, n2 = site["n1"], site["n2"]
    return {s: z_of(two_R(site["ref"][s], site["alt"][s]), n1, n2) for s in STATS}


def model(site):
    """The expected (mq_ranksum, rpr_ranksum, bq_ranksum) of a site."""
    z = site_z(site)
    return tuple(phred_of_z(z[s]) for s in STATS)


def z_class(z):
    """Name of the |z| class, or None.  z0 is exact; second_bottom excludes BRANCH and includes 7.6, above_cut excludes 37
    and includes 37.5, far excludes 38.5."""
    a = abs(z)
    if a == 0.0:
        return "z0"
    if 0.0 < a < 1.0:
        return "small"
    if 6.5 <= a < BRANCH:
        return "first_top"
    if BRANCH < a <= 7.6:
        return "second_bottom"
    if 14.0 <= a <= 16.0:
        return "mid15"
    if 29.0 <= a <= 31.0:
        return "mid30"
    if 36.5 <= a < CUT:
        return "below_cut"
    if CUT < a <= 37.5:
        return "above_cut"
    if a > 38.5:
        return "far"
    return None


def regime(z):
    """The path of bv_ranksum_phred / kf_erfc a z takes."""
    if z is None:
        return "no_z"
    a = abs(z)
    return "z0" if a == 0.0 else "first" if a < BRANCH else "second" if a <= CUT else "cut"


def clear_of_boundaries(z):
    return z is None or all(abs(abs(z) - b) > MARGIN * b for b in (CUT, BRANCH))


# ------------------------------------------------------------------------------------------------ classes
def _counts(vals):
    u, c = np.unique(np.asarray(vals, np.int64), return_counts=True)
    return dict(zip(u.tolist(), c.tolist()))


def layout_labels(site):
    """Where the values of the statistic under test sit: read off the site's reads."""
    s = site["stat"]
    L = set()
    r, a = _counts(site["ref"][s]), _counts(site["alt"][s])
    vals = sorted(set(r) | set(a))
    if not r or not a or len(vals) < 2:
        return L
    n = site["n1"] + site["n2"]
    for lo, hi in EDGE_PAIRS[s]:
        if vals == [lo, hi]:
            L.add("%s:edge:%d|%d" % (s, lo, hi))
    if s != "bq":
        wins = sorted({v // 64 for v in vals})
        if len(wins) == 1:
            L.add(s + ":window:same")
        if wins == [0, site["top"] // 64]:   # (the last window: of mapq 255, of the corpus's largest rank)
            L.add(s + ":window:empty_between")
        if len(vals) >= 3 and any(v in r and v in a and r[v] + a[v] >= n // 2 for v in vals):
            L.add(s + ":tie_block")
        if len(vals) >= 16 and len(wins) >= 2:
            L.add(s + ":ramp")
    else:
        if max(vals) == 93:
            L.add("bq:phred93")
        if list(r) == [41] and list(a) == [LOW_ALT_PHRED]:
            L.add("bq:ref41_alt_low")
    return L


def labels(site, rec):
    """The classes a site populates.  `rec`: the ORACLE's record of the site.  The read counts come from the record's
    depths, the z from the model; a |z| class counts only where the oracle's phred lies in the phred range of that class
    (10000 beyond the cut, a zero at z0), so a site that the oracle does not see as built populates nothing."""
    L = set()
    if (int(rec["status"]) & 0x12) != 0x12 or int(rec["n_alt"]) != 1 or int(rec["alt"][0]) != 1:
        return L
    if int(rec["depth"][0]) != site["n1"] or int(rec["depth"][1]) != site["n2"]:
        return L
    s = site["stat"]
    z = site_z(site)[s]
    ph = float(rec[FIELD[s]])
    if site.get("kind") == "qual":
        q = float(rec["qual"])
        for name, (lo, hi) in QUAL_CLASSES.items():
            if lo * (1 + MARGIN) <= q < hi * (1 - MARGIN):
                L.add(name)
        if site["name"].startswith("qual: first p = 0") and q == 10000.0:
            L.add("qual:zero")
        if site["name"].startswith("qual: neighbour below") and 2900.0 < q < QUAL_FLOOR:
            L.add("qual:zero_neighbour")
        return L
    if z is None:
        if ph == 10000.0:
            L.add("no_z")
        return L
    c = z_class(z)
    sign = "+" if z > 0 else "-"
    if c == "z0":
        if ph == 0.0:
            L.add("%s:z0:%s" % (s, "ties" if len(set(site["ref"][s]) | set(site["alt"][s])) == 1 else "untied"))
    elif c in ("above_cut", "far"):
        if ph == 10000.0:
            L.add("%s:%s:%s" % (s, c, sign))
    elif c is not None:
        lo, hi = Z_CLASSES[c]
        if phred_of_z(lo) * (1 - 1e-6) <= ph <= phred_of_z(min(hi, CUT)) * (1 + 1e-6):
            L.add("%s:%s:%s" % (s, c, sign))
    n = site["n1"] + site["n2"]
    if site.get("lopsided") == "few_alt" and site["n2"] * 8 < n:
        L.add(s + ":few_alt")
    if site.get("lopsided") == "few_ref" and site["n1"] * 8 < n:
        L.add(s + ":few_ref")
    L |= layout_labels(site)
    return L


def required_classes(n_samples, max_rank=65535):
    """Every class a corpus is asked to populate (what a row length cannot hold is subtracted by the caller)."""
    req = {"no_z"}
    for s in STATS:
        req |= {s + ":z0:ties", s + ":z0:untied", s + ":few_alt", s + ":few_ref"}
        req |= {"%s:%s:%s" % (s, c, sg) for c in Z_CLASSES for sg in "+-"}
        req |= {"%s:edge:%d|%d" % (s, lo, hi) for lo, hi in EDGE_PAIRS[s] if s != "rpr" or hi <= max_rank}
    for s in ("mq", "rpr"):
        req |= {s + ":window:same", s + ":window:empty_between", s + ":tie_block", s + ":ramp"}
    req |= {"bq:phred93", "bq:ref41_alt_low"}
    return req


def required_qual_classes():
    return set(QUAL_CLASSES) | {"qual:zero", "qual:zero_neighbour"}


# ------------------------------------------------------------------------------------------------ the corpus
class Corpus(list):
    """The sites of one row length: a list of site dicts, with `unreachable` (the targets the row length cannot hold, and
    why).  A site: name, stat (the statistic under test), n1 / n2 (REF / ALT reads), ref / alt ({statistic: one value per
    read}), optionally lopsided and kind."""

    def __init__(self, n_samples, max_rank):
        super().__init__()
        self.n_samples = n_samples
        self.max_rank = max_rank
        self.min_af = min_af(n_samples)
        self.unreachable = []

    @property
    def names(self):
        return [s["name"] for s in self]

    def add(self, name, stat, ref_vals, alt_vals, **kw):
        n1, n2 = len(ref_vals), len(alt_vals)
        if n1 + n2 > self.n_samples:
            self.unreachable.append("%s: needs %d reads" % (name, n1 + n2))
            return None
        top = {"mq": 255, "rpr": self.max_rank, "bq": 93}[stat]
        site = dict(name=name, stat=stat, n1=n1, n2=n2, top=top, ref={}, alt={}, **kw)
        for s in STATS:
            site["ref"][s] = np.minimum(np.asarray(ref_vals, np.int64), top) if s == stat else np.full(n1, CONST[s], np.int64)
            site["alt"][s] = np.minimum(np.asarray(alt_vals, np.int64), top) if s == stat else np.full(n2, CONST[s], np.int64)
        z = site_z(site)[stat]
        if not clear_of_boundaries(z):
            self.unreachable.append("%s: z = %.9g within %g of a branch boundary" % (name, z, MARGIN))
            return None
        self.append(site)
        return site


def nearest_two_value(n1, n2, target, cls=None):
    """(r_hi, a_hi, z): how many of n1 REF and n2 ALT reads hold the higher of two values so that z is nearest `target`
    (positive z: the REF reads rank lower, i.e. hold the lower values) and keeps MARGIN from the branch boundaries; with
    `cls`, the nearest point inside that |z| class where there is one."""
    den = 2.0 * math.sqrt(float(n1 * n2 * (n1 + n2 + 1)) / 12.0)
    best = None
    for r_hi in range(n1 + 1):
        a0 = int(round((target * den + n2 * r_hi) / n1))
        for a_hi in (a0 - 1, a0, a0 + 1):
            a_hi = min(max(a_hi, 0), n2)
            z = (n1 * a_hi - n2 * r_hi) / den
            if not clear_of_boundaries(z):
                continue
            # among equally near points, one that leaves both values on both classes of reads
            key = (cls is not None and z_class(z) != cls, round(abs(z - target), 9), abs(r_hi - n1 // 4))
            if best is None or key < best[0]:
                best = (key, r_hi, a_hi, z)
    return best[1:]


def two_value_reads(n1, n2, r_hi, a_hi, lo, hi):
    return [hi] * r_hi + [lo] * (n1 - r_hi), [hi] * a_hi + [lo] * (n2 - a_hi)


def ramp_reads(n1, n2, lo, hi, shift):
    """REF values spread evenly over lo..hi, ALT values over the same range shifted by `shift`."""
    ref = lo + (np.arange(n1, dtype=np.int64) * (hi - lo + 1)) // max(n1, 1)
    alt = lo + shift + (np.arange(n2, dtype=np.int64) * (hi - lo + 1)) // max(n2, 1)
    return ref.tolist(), alt.tolist()


def few_reads(n_samples, maf):
    """The read count of the small class of a lopsided site: a fifth above the smallest active depth of a full row, and six
    reads at least (fewer ALT reads on phred 20 are not called on a 60-sample row)."""
    return max(6, int(math.ceil(1.2 * maf * n_samples)) + 2)


@functools.lru_cache(maxsize=None)
def corpus(n_samples, max_rank=65535):
    """The sites of a row of n_samples (a Corpus, built once per row length and rank cap and shared: leave it unchanged).
    With max_rank = 8191 every rank fits the tagged layout (synth.tag_ranks): larger ranks are written as 8,191."""
    N = int(n_samples)
    C = Corpus(N, max_rank)
    m = min(1000, N // 2)
    n1, n2 = m, m - 1
    zmax = math.sqrt(3.0 * n1 * n2 / (n1 + n2 + 1))
    for s in STATS:
        pairs = PAIRS[s]
        k = 0

        def pair():
            nonlocal k
            k += 1
            return pairs[(k - 1) % len(pairs)]

        # ---- z exactly 0: every read ties; an untied arrangement R A A R over 4K distinct values (2R = n1 (n + 1))
        C.add("%s z0: every read ties" % s, s, [CONST[s]] * n1, [CONST[s]] * n2)
        K = min({"mq": 256, "rpr": 1200, "bq": 92}[s], N) // 4
        v = np.arange(4 * K) + (1 if s == "bq" else 0)
        inner = (np.arange(4 * K) % 4 == 1) | (np.arange(4 * K) % 4 == 2)
        C.add("%s z0: untied, symmetric" % s, s, v[~inner].tolist(), v[inner].tolist())
        # ---- the |z| classes, both signs, on two values
        for c, (zlo, zhi) in Z_CLASSES.items():
            for sg in (1, -1):
                name = "%s %s %s" % (s, c, "+" if sg > 0 else "-")
                if c == "far":
                    r_hi, a_hi, z = (0, n2, zmax) if sg > 0 else (n1, 0, -zmax)
                else:
                    r_hi, a_hi, z = nearest_two_value(n1, n2, sg * Z_TARGET[c], c)
                if z_class(z) != c or (z > 0) != (sg > 0):
                    C.unreachable.append("%s: %d + %d reads reach |z| = %.4g at most, nearest z = %.4g" % (name, n1, n2, zmax, z))
                    continue
                lo, hi = pair()
                C.add("%s (z = %.6g, %d | %d)" % (name, z, lo, hi), s, *two_value_reads(n1, n2, r_hi, a_hi, lo, hi))
        # ---- lopsided: the fewest reads of one class that are still called, beside all the row's other reads
        # (bq: on pairs of phred 20 and more, so that a handful of ALT reads is called whichever value they hold)
        few = few_reads(N, C.min_af)
        if s == "bq":
            pairs, k = [p for p in pairs if p[0] >= 20], 0
        for which, (a, b) in (("few_alt", (N - few, few)), ("few_ref", (few, N - few))):
            lo, hi = pair()
            r_hi, a_hi = (0, b) if which == "few_alt" else (a, 0)
            C.add("%s %s: %d + %d reads, separated (%d | %d)" % (s, which, a, b, lo, hi), s, *two_value_reads(a, b, r_hi, a_hi, lo, hi), lopsided=which)
            r_hi, a_hi, z = nearest_two_value(a, b, -3.0 if which == "few_alt" else 3.0)
            lo, hi = pair()
            C.add("%s %s: %d + %d reads, z = %.4g (%d | %d)" % (s, which, a, b, z, lo, hi), s, *two_value_reads(a, b, r_hi, a_hi, lo, hi), lopsided=which)
        # ---- every cell of the row a REF or an ALT read: the largest n1 n2 (n + 1) and the largest terms of 2R
        top = {"mq": 255, "rpr": max_rank, "bq": 93}[s]
        bot = 8 if s == "bq" else 0
        C.add("%s full row: %d + %d reads on a ramp" % (s, N - N // 2, N // 2), s, *ramp_reads(N - N // 2, N // 2, bot, top - 3, 3))
    # ---- where the values sit: mq and rpr
    for s, wsame, wfar, edge in (("mq", (70, 120), (9, 201), 191), ("rpr", (130, 190), (11, 65530), 1023)):
        r_hi, a_hi, z = nearest_two_value(n1, n2, 3.0)
        C.add("%s both values in one window (%d | %d)" % ((s,) + wsame), s, *two_value_reads(n1, n2, r_hi, a_hi, *wsame))
        C.add("%s first and last window, empty windows between (%d | %d)" % ((s,) + wfar), s, *two_value_reads(n1, n2, r_hi, a_hi, *wfar))
        for lo, hi in EDGE_PAIRS[s]:
            r_hi, a_hi, z = nearest_two_value(n1, n2, -2.0)
            C.add("%s pair across a window edge (%d | %d)" % (s, lo, hi), s, *two_value_reads(n1, n2, r_hi, a_hi, lo, hi))
        # a tie block that REF and ALT share (t_v = 60 % of the reads) beside a separated remainder
        t1, t2 = n1 * 6 // 10, n2 * 6 // 10
        for sg, (rv, av) in ((1, (edge - 40, edge + 40)), (-1, (edge + 40, edge - 40))):
            C.add("%s shared tie block on %d, REF rest on %d, ALT rest on %d" % (s, edge, rv, av), s,
                  [edge] * t1 + [rv] * (n1 - t1), [edge] * t2 + [av] * (n2 - t2))
        for shift in (5, -5):
            C.add("%s ramp across %d | %d, ALT shifted by %d" % (s, edge, edge + 1, shift), s, *ramp_reads(n1, n2, edge - 30, edge + 30, shift))
    # ---- bq: the 16-value windows, phred 93, REF on phred 41 against ALT on a low phred
    for lo, hi in EDGE_PAIRS["bq"]:
        r_hi, a_hi, z = nearest_two_value(n1, n2, -2.0)
        C.add("bq pair across a window edge (%d | %d)" % (lo, hi), "bq", *two_value_reads(n1, n2, r_hi, a_hi, lo, hi))
    C.add("bq ramp over phred 10..93", "bq", *ramp_reads(n1, n2, 10, 90, 3))
    C.add("bq REF on phred 41, ALT on phred %d" % LOW_ALT_PHRED, "bq", [41] * n1, [LOW_ALT_PHRED] * n2)
    # ---- no z: a variant site without a REF read (10000 through n1 == 0), between sites of other regimes
    for j in range(1, 8):
        C.insert(j * len(C) // 8, _no_ref_site(n2 - j, "no z: no REF read (%d)" % j))
    C.append(_no_ref_site(min(N, 64), "no z: no REF read (shallow)"))
    return C


def _no_ref_site(n2, name="no z: no REF read"):
    return dict(name=name, stat="mq", n1=0, n2=n2, ref={s: np.zeros(0, np.int64) for s in STATS},
                alt={"mq": np.arange(n2, dtype=np.int64) % 61, "rpr": 1 + np.arange(n2, dtype=np.int64) % 150,
                     "bq": 20 + np.arange(n2, dtype=np.int64) % 21})


# ------------------------------------------------------------------------------------------------ QUAL at a chosen chi2
def _qual_site(name, n_ref, alt_phreds):
    n2 = len(alt_phreds)
    site = dict(name=name, stat="bq", kind="qual", n1=n_ref, n2=n2, ref={}, alt={})
    for s in STATS:
        site["ref"][s] = np.full(n_ref, (35 if n_ref > 64 else 93) if s == "bq" else CONST[s], np.int64)
        site["alt"][s] = np.asarray(alt_phreds, np.int64) if s == "bq" else np.full(n2, CONST[s], np.int64)
    return site


_qual_cache = {}


def qual_sites(oracle, n_samples):
    """Two-base sites at a chosen QUAL: REF reads on phred 35, and k ALT reads on phred 93 (about 95 of QUAL each) with up
    to four on phred 20 (about 20 each), swept against the oracle's QUAL (-10 log10 of the chi2 tail) on a short row.  Kept:
    the site nearest the middle of each range of QUAL_CLASSES, the first site of the sweep whose p is exactly 0 (QUAL
    10000) and, as its neighbour below, the last one whose p keeps 34 bits (QUAL < 3130.7).  Returns (sites, excluded):
    the sites between those two, whose p is a denormal of fewer bits, are named in `excluded` and left out, and so is
    every class that the sweep does not reach.  Rows of more than 64 samples hold 200 REF reads.  Rows of 60 samples hold
    30 REF reads on phred 93 and at most 30 ALT reads (a shallow site: the per-sample replay); the statistic is that of
    dropping the weaker of the two bases, so 60 reads end near QUAL 2,700 and the classes beyond are out of their reach."""
    N = int(n_samples)
    n_ref = 30 if N <= 64 else 200
    if n_ref not in _qual_cache:
        cand = [(k, j) for k in range(0, 45 if n_ref > 64 else 27) for j in range(5) if k + j >= 4 or (k >= 1 and n_ref <= 64)]
        W = 256
        sw = [_qual_site("sweep", n_ref, [93] * k + [20] * j) for k, j in cand]
        e, _ = oracle.run(slab(sw, W), min_af(W), n_threads=8)
        _qual_cache[n_ref] = (cand, e["qual"].copy(), (e["status"] & 2) != 0)
    cand, q, variant = _qual_cache[n_ref]
    order = [i for i in np.argsort(q, kind="stable") if variant[i]]
    sites, excluded = [], []
    for name, (lo, hi) in QUAL_CLASSES.items():
        inside = [i for i in order if lo * (1 + 1e-3) <= q[i] < hi * (1 - 1e-3)]
        if inside:
            i = min(inside, key=lambda i: abs(q[i] - (lo + hi) / 2))
            k, j = cand[i]
            sites.append(_qual_site("%s (%d on phred 93, %d on phred 20)" % (name, k, j), n_ref, [93] * k + [20] * j))
        else:
            excluded.append("%s: the sweep beside %d REF reads ends at QUAL %.1f" % (name, n_ref, max(q[i] for i in order)))
    zero = [i for i in order if q[i] == 10000.0]
    if not zero:
        excluded.append("qual:zero and its neighbour: the sweep beside %d REF reads ends at QUAL %.1f" % (n_ref, max(q[i] for i in order)))
    else:
        below = [i for i in order if q[i] < QUAL_FLOOR * (1 - 1e-3)]
        k, j = cand[zero[0]]
        sites.append(_qual_site("qual: first p = 0 (%d on phred 93, %d on phred 20)" % (k, j), n_ref, [93] * k + [20] * j))
        k, j = cand[below[-1]]
        sites.append(_qual_site("qual: neighbour below p = 0 with 34 bits (%d on phred 93, %d on phred 20)" % (k, j), n_ref, [93] * k + [20] * j))
        excluded += ["QUAL %.1f (%d on phred 93, %d on phred 20): p a denormal of fewer than 34 bits" % (q[i], cand[i][0], cand[i][1])
                     for i in order if QUAL_FLOOR * (1 - 1e-3) <= q[i] < 10000.0]
    return sites, excluded


# ------------------------------------------------------------------------------------------------ the slab
def slab(sites, n_samples, order=None):
    """One site per entry: REF A, ALT C, strands alternating read by read, the reads on cells drawn by a permutation seeded
    by the site's index, every other cell uncovered.  `order`: site i of the slab is entry order[i] -- its reads move with
    it.  Cells past n_samples look covered."""
    S, N = len(sites), int(n_samples)
    pitch = (N + 15) // 16 * 16
    out = {"n_sites": S, "n_samples": N, "pitch": pitch, "n_groups": 0,
           "base_strand": np.full((S, pitch), 8, np.uint8), "qual": np.zeros((S, pitch), np.uint8),
           "mapq": np.zeros((S, pitch), np.uint8), "rpr": np.zeros((S, pitch), np.uint16), "ref_base": np.zeros(S, np.uint8)}
    out["base_strand"][:, N:] = 0; out["qual"][:, N:] = 40; out["mapq"][:, N:] = 60; out["rpr"][:, N:] = 7
    for i, site in enumerate(sites):
        n1, n2 = site["n1"], site["n2"]
        assert n1 + n2 <= N, site["name"]
        cells = np.random.default_rng([N, i, 0x5A]).permutation(N)[:n1 + n2]
        strand = ((np.arange(n1 + n2) & 1) << 2).astype(np.uint8)
        out["base_strand"][i, cells] = np.concatenate([np.zeros(n1, np.uint8), np.ones(n2, np.uint8)]) | strand
        for s in STATS:
            out[PLANE[s]][i, cells] = np.concatenate([site["ref"][s], site["alt"][s]])
    if order is not None:
        order = np.asarray(order)
        assert sorted(order.tolist()) == list(range(S))
        for k in ("base_strand", "qual", "mapq", "rpr"):
            out[k] = np.ascontiguousarray(out[k][order])
    return out


# ------------------------------------------------------------------------------------------------ regimes on adjacent sites
def regime_pairs(regimes, order):
    """{(statistic, regime of site order[i], regime of site order[i + 1])}."""
    return {(s, regimes[a][s], regimes[b][s]) for a, b in zip(order[:-1], order[1:]) for s in STATS}


def orders(sites, tries=32):
    """([identity, reversed, a seeded permutation], pairs, wanted): `pairs` are the (statistic, regime, regime) triples the
    three orders put on adjacent sites, `wanted` every ordered pair of the regimes that the sites of a statistic show.  The
    permutation is a chain: from a seeded shuffle of the sites, the next site is the one that puts the most wanted pairs
    not seen so far beside the last one; of `tries` seeds the chain that leaves the fewest wanted pairs out is kept (none,
    on every row length of the tests).  A MODEL of the one-site-per-lane finish: see the module's docstring."""
    regimes = []
    for site in sites:
        z = site_z(site)
        regimes.append({s: regime(z[s]) for s in STATS})
    S = len(sites)
    wanted = set()
    for s in STATS:
        have = {r[s] for r in regimes}
        wanted |= {(s, a, b) for a in have for b in have}
    base = [np.arange(S), np.arange(S)[::-1].copy()]
    seen = regime_pairs(regimes, base[0]) | regime_pairs(regimes, base[1])
    best = None
    for t in range(tries):
        left = np.random.default_rng(2000 + t).permutation(S).tolist()
        chain, missing = [left.pop(0)], set(wanted - seen)
        while left:
            a = chain[-1]
            gain = [sum((s, regimes[a][s], regimes[b][s]) in missing for s in STATS) for b in left]
            b = left.pop(int(np.argmax(gain)))
            missing -= {(s, regimes[a][s], regimes[b][s]) for s in STATS}
            chain.append(b)
        if best is None or len(missing) < best[0]:
            best = (len(missing), np.asarray(chain), seen | regime_pairs(regimes, chain))
        if not missing:
            break
    return base + [best[1]], best[2], wanted
