"""Strand-bias tables built by construction for the Fisher tests of short and long rows (a test helper, not a conftest).

FS and SOR of a short row (<= 49,152 samples) come from one of three realisations of kt_fisher_exact: the 16-lane form
with its three regimes (candidates, four sites to a wave), the one-lane serial walk (hom-ref sites of at most 32 tables)
and the wave form (shallow sites, phred-0 calls, every long row).  Slabs with coin-flip strands only ever show them
balanced tables with p near 1.  Here the tables are computed from targets -- a table count R, where the observed table
sits in its family, how unlikely it is -- and sized to the reads a row length holds:

  classify()   a plain-Python restatement of the routing (which realisation, which regime), written from the comments of
               the kernels and sharing no code with them;
  corpus()     the tables of one row length, with the targets that row length cannot reach named, never dropped;
  slab()       one site per table, in a given order of the sites;
  labels()     the classes a classified table belongs to, required_classes() the classes a corpus must populate;
  exact_two_sided()   the two-sided rule in 60-digit decimal arithmetic over an exact hypergeometric pmf;
  serial_walk()       the rule as htslib walks it, in Python's doubles.

Long rows (> 49,152 samples), tile jobs and the shallow / phred-0 sites of short rows take the wave form, whose boundaries
are its own -- one table per lane up to 64, rounds of 64 without probes up to 256, probes at span // 63 + 1 beyond:

  classify_wave()   a plain-Python model of that walk (regime, probe steps, window, rounds, lanes, shift, live floor);
  corpus_long()     corpus() plus the wave-form targets, for the row lengths of LONG_ROWS; corpus_million() a short list
                    at 1,000,000 samples;
  wave_labels(), required_wave_classes(), wave_site_classes()   the classes of those targets.

BV_SITE_SOR_OVERFLOW needs a product of two cells above 2^31, i.e. more than 92,682 reads in a row, and a product that
wraps to 0 more than 131,072: out of reach of short rows, they are in the long corpora (the SOR tables of _add_wave_tables)
and in tests/golden/deep_sor.npz and sor_wrap.npz.
"""
import decimal
import functools
import math

import numpy as np

SHORT_ROW_MAX = 49152   # rows of more samples take the long-row kernel (the wave form everywhere)
LANE_MAX_TABLES = 32    # a hom-ref site of more tables goes to the 16-lane solver
PRODUCT_MAX_MARGIN = 12  # a row margin of at most this many reads: product form
NARROW_MAX_TABLES = 128  # more tables: tail probes
SHALLOW_MAX = 64        # sites of at most this many covered samples are replayed by the wave solver
LOG10_2 = math.log10(2.0)
P_FLOOR_LOG10 = -1040 * LOG10_2   # below 2^-1040 a double keeps fewer than 34 bits
ZERO_LOG10 = -326.0     # log10 q below this: exp() gives exactly 0

TIE_K = (1, 8, 64)
UNDERFLOW_K = (505, 513, 515, 522, 560)
PRODUCT_MARGINS = (11, 12, 13)
LANE_R = (2, 11, 12, 22, 31, 32)
NARROW_R = (14, 16, 17, 64, 65, 127, 128)
PROBED_R = (129, 130, 256, 257)
END_STEPS = (1, 14, 15, 16)   # tables between the observed one and an end: span / 15 + 1 goes from 1 to 2 at 15
SKEWS = {"q2": (-4.0, -1.3), "q20": (-30.0, -14.0), "q200": (-290.0, -140.0), "q300": (-308.0, -292.0)}
SKEW_TARGET = {"q2": -2.0, "q20": -20.0, "q200": -200.0, "q300": -300.0}
Q150 = (-153.0, -135.0)   # q just above 2^-511 (log10 = -153.8): the smallest q that the kernels carry unscaled
STEEP_R = (129, 256)      # families whose first table lies below the double range beside an ordinary q
STEEP_LOG = -760.0        # ln p of that first table: exp() gives 0 (the smallest double is e^-744.4)


def min_af(n_samples, user_min_af=0.01):
    """(double)std::min(float(100) / n, min_af) of the caller, in float arithmetic."""
    return float(min(np.float32(100.0) / np.float32(n_samples), np.float32(user_min_af)))


def _lbinom(n, k):
    return math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)


def family(t):
    """(imin, imax, n1_, n_1, n) of the table family of t = (n11, n12, n21, n22)."""
    n11, n12, n21, n22 = t
    n1_, n_1, n = n11 + n12, n11 + n21, n11 + n12 + n21 + n22
    return max(0, n1_ + n_1 - n), min(n1_, n_1), n1_, n_1, n


def log10_q(t):
    """log10 of the observed table's hypergeometric probability, from math.lgamma."""
    _, _, n1_, n_1, n = family(t)
    return (_lbinom(n1_, t[0]) + _lbinom(n - n1_, t[2]) - _lbinom(n, n_1)) / math.log(10.0)


def classify(table, n_samples, min_af, depths=None, phred0=False):
    """Where the Fisher test of one (ref_fwd, ref_rev, alt_fwd, alt_rev) table is computed on a row of n_samples.

    `depths`: the site's reads per base, REF first (default: one ALT base holding the table's ALT row); `phred0`: the site
    has a phred-0 call.  A site is a short-row candidate unless exactly one base reaches min_af, that base is REF, no call
    has phred 0 and the table family has at most 32 tables; non-candidates are finished by one lane each.  Candidates go
    four to a wave onto groups of 16 lanes, where a row margin of at most 12 takes the product form, up to 128 tables the
    narrow seeds and more tables the tail probes -- unless the site is shallow (<= 64 reads) or has a phred-0 call, which
    keep the one-site-per-wave solver, as every site of a long row does.

    `lane` is tested before `product`: a non-candidate never reaches the 16-lane solver, so a hom-ref site with a row margin
    of at most 12 is walked by one lane and is no product-form table.  (Read as a list of definitions, the regimes are:
    degenerate imin == imax; lane not a candidate; product m <= 12; narrow R <= 128; probed R > 128.)"""
    rf, rr, af, ar = (int(x) for x in table)
    imin, imax, n1_, n_1, n = family((rf, rr, af, ar))
    R = imax - imin + 1
    m = min(n1_, n - n1_)
    if depths is None:
        depths = (rf + rr, af + ar)
    total = sum(int(d) for d in depths)
    active = [total > 0 and int(d) / total >= min_af for d in depths]
    hom_ref = sum(active) == 1 and active[0]
    candidate = total > 0 and (not hom_ref or phred0 or R > LANE_MAX_TABLES)
    if imin == imax:
        regime = "degenerate"
    elif not candidate:
        regime = "lane"
    elif m <= PRODUCT_MAX_MARGIN:
        regime = "product"
    elif R <= NARROW_MAX_TABLES:
        regime = "narrow"
    else:
        regime = "probed"
    if n_samples > SHORT_ROW_MAX or (candidate and (phred0 or total <= SHALLOW_MAX)):
        solver = "wave"
    else:
        solver = "g16" if candidate else "lane"
    n_2 = n - n_1
    return {"R": R, "m": m, "log10q": log10_q((rf, rr, af, ar)), "regime": regime, "imin": imin, "imax": imax,
            "position": "imin" if rf == imin else "imax" if rf == imax else "interior",
            "candidate": candidate, "hom_ref": hom_ref, "n_active": sum(active), "solver": solver,
            "jmin": max(0, m - n_2), "small_row": "alt" if n - n1_ <= n1_ else "ref"}


# ------------------------------------------------------------------------------------------------ the wave form
WAVE = 64                  # tables per round: one per lane
WAVE_ROUNDS_MAX = 256      # more tables: a probe of log p per lane on either side first
WAVE_PROBES = 63           # steps between the probe points of a side
CUT_NATS = 60.0            # a tail below q * e^-60 is skipped
SHIFT_LOG = -354.0         # ln q below this: the family is carried scaled by 2^512
SHIFT = 512 * math.log(2.0)
LIVE_FLOOR = -700.0        # a walk whose first table has ln p + shift below this starts at the first table that reaches it
LNFACT_TABLE_MIN = 65536   # the engine's log-factorial table never has fewer entries; arguments beyond a table take the series
EXP_ZERO = -745.14         # exp() of less is 0


def log_p(t, i):
    """ln of the hypergeometric probability of the table n11 = i in the family of t, from math.lgamma."""
    _, _, n1_, n_1, n = family(t)
    return _lbinom(n1_, i) + _lbinom(n - n1_, n_1 - i) - _lbinom(n, n_1)


def classify_wave(table):
    """How the wave form (one family on the 64 lanes of a wave: every site of a long row, every tile job, shallow and
    phred-0 sites of short rows) walks one (n11, n12, n21, n22) table: a plain-Python model written from the comments of
    csrc/bv_fisher.h, sharing no code with the kernels.

    regime      degenerate (imin == imax), product (a row margin <= 12), lanes (R <= 64: one table per lane),
                rounds (65..256: rounds of 64 tables over the whole family), probed (> 256: tails skipped first);
    q0          rounds / probed: exp(ln q) is 0, the test returns before any walk (the keys below are then absent);
    steps       probed: (span // 63 + 1) of [imin, n11] and of [n11, imax];
    probe_window  probed: [wl, wr] as the probes leave it -- wl the last probe point of the left side below
                ln q - 60, wr the first of the right side;
    shifted     ln q < -354: every table carried scaled by 2^512;
    below_floor the first table of the window has ln p + shift < -700: the walk starts at the first live table instead;
    window      [wl, wr] as walked; rounds: its rounds of 64; lane: the lane of the observed table in its round;
    lstar, rstar  the first table from the left / right with p >= 0.99999999 q; same_round: both in one round;
    series      some log-factorial argument reaches 65,536 (beyond the smallest table the engine builds);
    series_mixed  the four cells of the observed table lie on both sides of 65,536: one log p mixes table and series."""
    t = tuple(int(x) for x in table)
    n11 = t[0]
    imin, imax, n1_, n_1, n = family(t)
    R = imax - imin + 1
    m = min(n1_, n - n1_)
    args = (n1_, n - n1_, n, n_1, n - n_1) + t
    out = {"R": R, "m": m, "imin": imin, "imax": imax, "series": max(args) >= LNFACT_TABLE_MIN,
           "series_mixed": max(t) >= LNFACT_TABLE_MIN > min(t)}
    if imin == imax:
        out["regime"] = "degenerate"
        return out
    if m <= PRODUCT_MAX_MARGIN:
        out.update(regime="product", rounds=1)
        return out
    if R <= WAVE:
        out.update(regime="lanes", rounds=1, lane=n11 - imin, window=(imin, imax))
        return out
    out["regime"] = "rounds" if R <= WAVE_ROUNDS_MAX else "probed"
    lq = log_p(t, n11)
    out["q0"] = lq < EXP_ZERO
    if out["q0"]:
        return out
    shift = SHIFT if lq < SHIFT_LOG else 0.0
    wl, wr = imin, imax
    if out["regime"] == "probed":
        cut = lq - CUT_NATS
        sl, sr = (n11 - imin) // WAVE_PROBES + 1, (imax - n11) // WAVE_PROBES + 1
        below = [i for i in (imin + g * sl for g in range(WAVE)) if i <= n11 and log_p(t, i) < cut]
        if below:
            wl = max(below)
        below = [i for i in (imax - g * sr for g in range(WAVE)) if i >= n11 and log_p(t, i) < cut]
        if below:
            wr = min(below)
        out.update(steps=(sl, sr), probe_window=(wl, wr))
    mode = (n1_ + 1) * (n_1 + 1) // (n + 2)
    out["shifted"] = shift != 0.0
    out["below_floor"] = log_p(t, wl) + shift < LIVE_FLOOR
    if out["below_floor"]:
        top = min(wr, mode)
        if wl < top:
            lo, hi = wl + 1, top
            while lo < hi:
                mid = lo + (hi - lo) // 2
                if log_p(t, mid) + shift >= LIVE_FLOOR:
                    hi = mid
                else:
                    lo = mid + 1
            wl = lo
    # L* / R*: the pmf is unimodal, the tables of at least 0.99999999 q are those of one interval around n11 and the mode
    lo_log = lq + math.log(0.99999999)
    a, b = wl, max(wl, min(n11, mode))
    while a < b:
        mid = (a + b) // 2
        if log_p(t, mid) >= lo_log:
            b = mid
        else:
            a = mid + 1
    lstar = min(a, n11)
    a, b = min(wr, max(n11, mode)), wr
    while a < b:
        mid = (a + b + 1) // 2
        if log_p(t, mid) >= lo_log:
            a = mid
        else:
            b = mid - 1
    rstar = max(a, n11)
    out.update(window=(wl, wr), rounds=(wr - wl) // WAVE + 1, lane=(n11 - wl) % WAVE, lstar=lstar, rstar=rstar,
               same_round=(lstar - wl) // WAVE == (rstar - wl) // WAVE)
    return out


WAVE_R = (2, 63, 64, 65, 255, 256, 257)
WAVE_SPANS = (62, 63, 64)          # span // 63 + 1 goes from 1 to 2 at 63
WAVE_STEEP_R = (3001, 20001)
FAR_ROUNDS = 8                     # L* and R* at least this many rounds apart
LONG_WINDOW_ROUNDS = 100
SOR_PAIRS = {(46340, 46341): "46340x46341", (46341, 46341): "46341x46341", (65535, 65537): "65537x65535",
             (65537, 65537): "65537x65537"}


def wave_labels(t, w):
    """The wave-form classes of table t with the model's account w (classify_wave)."""
    rf, rr, af, ar = (int(x) for x in t)
    L = set()
    reg = w["regime"]
    if reg in ("lanes", "rounds", "probed") and w["R"] in WAVE_R:
        L.add("wave:R=%d:%s" % (w["R"], reg))
    if reg == "probed":
        for side, d in (("left", rf - w["imin"]), ("right", w["imax"] - rf)):
            if d in WAVE_SPANS:
                L.add("wave:span:%s=%d:%s" % (side, d, "q0" if w["q0"] else "live"))
    if reg in ("rounds", "probed") and not w["q0"]:
        wl, wr = w["window"]
        if (wr - wl + 1) % WAVE in (0, 1, 63):
            L.add("wave:window%%64=%d" % ((wr - wl + 1) % WAVE))
        if w["lane"] in (0, 63):
            L.add("wave:lane=%d" % w["lane"])
        if w["same_round"]:
            L.add("wave:LR:same_round")
        elif (w["rstar"] - wl) // WAVE - (w["lstar"] - wl) // WAVE >= FAR_ROUNDS:
            L.add("wave:LR:far_apart")
        if w["rounds"] >= LONG_WINDOW_ROUNDS:
            L.add("wave:rounds>=100")
        if reg == "probed" and w["R"] in WAVE_STEEP_R and 4 * w["m"] <= sum(t) and min(log_p(t, w["imin"]), log_p(t, w["imax"])) < STEEP_LOG:
            _, _, n1_, n_1, n = family(t)
            if abs(rf - (n1_ + 1) * (n_1 + 1) // (n + 2)) <= 1:
                L.add("wave:steep:R=%d" % w["R"])
        if reg == "probed" and w["below_floor"] and w["shifted"] and w["probe_window"][0] > w["imin"]:
            L.add("wave:shifted_below_floor_after_probe")
        if w["series_mixed"]:
            L.add("wave:series_mixed")
    num, den = tuple(sorted((rf, ar))), tuple(sorted((rr, af)))
    if num in SOR_PAIRS:
        L.add("sor:num=" + SOR_PAIRS[num])
    if den in SOR_PAIRS:
        L.add("sor:den=" + SOR_PAIRS[den])
    nz, dz = rf * ar > 0 and rf * ar % 2 ** 32 == 0, rr * af > 0 and rr * af % 2 ** 32 == 0
    if dz:
        L.add("sor:wrap0:" + ("both" if rf * ar == 0 else "den"))
    elif nz:
        L.add("sor:wrap0:num")
    return L


def required_wave_classes():
    """Every wave-form class a long corpus is asked to populate (what a length cannot hold is subtracted by the caller)."""
    req = {"wave:R=%d:%s" % (R, "lanes" if R <= WAVE else "rounds" if R <= WAVE_ROUNDS_MAX else "probed") for R in WAVE_R}
    req |= {"wave:span:%s=%d:%s" % (s, d, q) for s in ("left", "right") for d in WAVE_SPANS for q in ("live", "q0")}
    req |= {"wave:window%64=0", "wave:window%64=1", "wave:window%64=63", "wave:lane=0", "wave:lane=63", "wave:LR:same_round",
            "wave:LR:far_apart", "wave:rounds>=100", "wave:shifted_below_floor_after_probe", "wave:series_mixed"}
    req |= {"wave:steep:R=%d" % R for R in WAVE_STEEP_R}
    req |= {"sor:%s=%s" % (s, p) for s in ("num", "den") for p in ("46340x46341", "46341x46341")}
    req |= {"sor:den=65537x65535", "sor:den=65537x65537", "sor:wrap0:den", "sor:wrap0:num", "sor:wrap0:both", "sor:vcf_cvg_differ"}
    return req


def overflows(t):
    """BV_SITE_SOR_OVERFLOW of one four-column table: a product of SOR's quotient is above 2^31 - 1."""
    return t[0] * t[3] > 0x7fffffff or t[1] * t[2] > 0x7fffffff


def wave_site_classes(exp):
    """The wave-form classes the oracle's records `exp` of a long corpus slab populate: every CVG table, every VCF table of
    a variant site, and the site whose two tables differ in BV_SITE_SOR_OVERFLOW."""
    got = set()
    for rec in exp:
        cv = tuple(int(x) for x in rec["cvg_sb"])
        got |= wave_labels(cv, classify_wave(cv))
        if rec["n_alt"] > 0:
            vv = tuple(int(x) for x in rec["var_sb"])
            if vv != cv:
                got |= wave_labels(vv, classify_wave(vv))
                if overflows(vv) != overflows(cv):
                    got.add("sor:vcf_cvg_differ")
    return got


# ------------------------------------------------------------------------------------------------ classes
def labels(t, c, n_samples):
    """The classes of the corpus that table t with classification c (classify) belongs to."""
    rf, rr, af, ar = (int(x) for x in t)
    L = set()
    reg, R, m, lq = c["regime"], c["R"], c["m"], c["log10q"]
    lo, hi = c["imin"], c["imax"]
    if c["candidate"] and m in PRODUCT_MARGINS and reg == ("product" if m <= PRODUCT_MAX_MARGIN else "narrow"):
        L.add("margin%d:%s:%s" % (m, c["small_row"], c["position"]))
    if reg == "product" and c["jmin"] > 0:
        L.add("product:jmin>0:" + c["small_row"])
    if reg == "lane":
        if R in LANE_R:
            L.add("lane:R=%d" % R)
        if lo % 11 == 0:
            L.add("lane:mult11:first")
        if hi % 11 == 0:
            L.add("lane:mult11:last")
        if (lo // 11 + 1) * 11 < hi:
            L.add("lane:mult11:middle")
        L.add("lane:imin>0" if lo > 0 else "lane:imin=0")
        if c["position"] != "interior":
            L.add("lane:at_" + c["position"])
        if af + ar > 0 and (af == 0 or ar == 0):
            L.add("lane:one_strand_alt")
    if c["hom_ref"] and R == LANE_MAX_TABLES + 1 and reg == "narrow":
        L.add("homref:R=33:g16")
    skew = [k for k, (a, b) in SKEWS.items() if a <= lq <= b]
    if reg == "narrow":
        if R in NARROW_R:
            L.add("narrow:R=%d" % R)
        if lq > -1.3:
            L.add("narrow:balanced")
        L.update("narrow:" + k for k in skew if k != "q300")
    if reg == "probed":
        if R in PROBED_R:
            L.add("probed:R=%d" % R)
        if 900 <= R <= 1100:
            L.add("probed:R~1000")
        if R == n_samples // 2 + 1:
            L.add("probed:R=max")
        _, _, n1_, n_1, n = family((rf, rr, af, ar))
        if abs(rf - (n1_ + 1) * (n_1 + 1) // (n + 2)) <= 1:
            L.add("probed:mode")
        live = lq > -300.0
        for side, d in (("left", rf - lo), ("right", hi - rf)):
            if d == 0 or d in END_STEPS:
                L.add("probed:%s+%d" % (side, d))
                if live and d:
                    L.add("probed:%s+%d:live" % (side, d))
        if rr == 0 and af == 0 and rf == ar:
            L.add("probed:k00k")
        if rf == 0 and ar == 0 and rr == af:
            L.add("probed:0kk0")
        L.update("probed:" + k for k in skew if k != "q300")
        if Q150[0] <= lq <= Q150[1] and c["position"] == "interior" and R == n_samples // 2 + 1:
            L.add("probed:q150:" + ("left" if 2 * rf < lo + hi else "right"))
        if "q300" in skew and c["position"] == "interior":
            L.add("probed:q300:" + ("left" if 2 * rf < lo + hi else "right"))
    if c["candidate"] and R in STEEP_R and lq > -10.0:
        ends = [e for e, i in (("imin", lo), ("imax", hi)) if log10_q((i, rf + rr - i, rf + af - i, ar - rf + i)) * math.log(10.0) < STEEP_LOG]
        L.update("steep_end:R=%d:%s" % (R, e) for e in ends)
    for k in TIE_K:
        if (rf, rr, af, ar) == (k, k, k, k):
            L.add("tie:kkkk:%d" % k)
        if (rf, rr, af, ar) == (k, 0, 0, k):
            L.add("tie:k00k:%d" % k)
    for k in UNDERFLOW_K:
        if (rf, rr, af, ar) == (k, 0, 0, k):
            L.add("underflow:k=%d" % k)
    if rr == 0 and af == 0:
        L.add("sor:both=0")
    elif rr == 0:
        L.add("sor:ref_rev=0")
    elif af == 0:
        L.add("sor:alt_fwd=0")
    elif rr == 1 and af == 1:
        L.add("sor:one_read_cells")
    if reg == "degenerate":
        L.add("degenerate:" + c["solver"])
    if c["candidate"] and reg != "degenerate" and lq < ZERO_LOG10:
        L.add("q0:" + c["solver"])
    return L


def required_classes(n_samples):
    """Every class a corpus is asked to populate (what a row length cannot hold is subtracted by the caller)."""
    solver = "wave" if n_samples > SHORT_ROW_MAX else "g16"
    req = {"margin%d:%s:%s" % (m, row, pos) for m in PRODUCT_MARGINS for row in ("alt", "ref") for pos in ("imin", "imax", "interior")}
    req |= {"product:jmin>0:alt", "product:jmin>0:ref"}
    req |= {"lane:R=%d" % R for R in LANE_R} | {"homref:R=33:g16"}
    req |= {"lane:mult11:first", "lane:mult11:last", "lane:mult11:middle", "lane:imin>0", "lane:imin=0", "lane:at_imin",
            "lane:at_imax", "lane:one_strand_alt"}
    req |= {"narrow:R=%d" % R for R in NARROW_R} | {"narrow:balanced", "narrow:q2", "narrow:q20", "narrow:q200"}
    req |= {"probed:R=%d" % R for R in PROBED_R} | {"probed:R~1000", "probed:R=max", "probed:mode", "probed:k00k", "probed:0kk0"}
    req |= {"probed:%s+%d" % (s, d) for s in ("left", "right") for d in (0,) + END_STEPS}
    req |= {"probed:%s+%d:live" % (s, d) for s in ("left", "right") for d in END_STEPS}
    req |= {"probed:q2", "probed:q20", "probed:q200", "probed:q300:left", "probed:q300:right", "probed:q150:left", "probed:q150:right"}
    req |= {"steep_end:R=%d:%s" % (R, e) for R in STEEP_R for e in ("imin", "imax")}
    req |= {"tie:kkkk:%d" % k for k in TIE_K} | {"tie:k00k:%d" % k for k in TIE_K}
    req |= {"underflow:k=%d" % k for k in UNDERFLOW_K}
    req |= {"sor:both=0", "sor:ref_rev=0", "sor:alt_fwd=0", "sor:one_read_cells"}
    req |= {"degenerate:" + solver, "degenerate:" + ("wave" if n_samples > SHORT_ROW_MAX else "lane"), "q0:" + solver}
    req |= {"site:two_regimes", "site:same_shortcut"}
    return req


def site_classes(exp, n_samples, maf):
    """The classes the oracle's records `exp` of a corpus slab populate: every CVG table, every VCF table of a variant
    site, and the two site classes of the six-column tables."""
    got = set()
    for rec in exp:
        depths = [int(d) for d in rec["depth"]]   # REF is base 0 in every corpus site
        cv = tuple(int(x) for x in rec["cvg_sb"])
        c = classify(cv, n_samples, maf, depths=depths)
        got |= labels(cv, c, n_samples)
        if rec["n_alt"] > 0:
            vv = tuple(int(x) for x in rec["var_sb"])
            if vv == cv:
                if rec["n_alt"] == 2:
                    got.add("site:same_shortcut")
            else:
                v = classify(vv, n_samples, maf, depths=depths)   # (a called ALT base is active: a candidate)
                got |= labels(vv, v, n_samples)
                if v["regime"] != c["regime"]:
                    got.add("site:two_regimes")
    return got


# ------------------------------------------------------------------------------------------------ the corpus
class Corpus(list):
    """The tables of one row length: a list of 4- or 6-column tables, with `names` (the builder's intent per table) and
    `unreachable` (the targets the row length cannot hold, and why)."""

    def __init__(self, n_samples):
        super().__init__()
        self.n_samples = n_samples
        self.min_af = min_af(n_samples)
        self.names = []
        self.unreachable = []

    def add(self, name, t):
        t = tuple(int(x) for x in t)
        if min(t) < 0 or sum(t) > self.n_samples:
            self.unreachable.append("%s: needs %d reads" % (name, sum(t)) if min(t) >= 0 else "%s: no such table" % name)
            return False
        t6 = t + (0, 0)
        lq = log10_q((t6[0], t6[1], t6[2] + t6[4], t6[3] + t6[5]))
        if ZERO_LOG10 <= lq < P_FLOOR_LOG10:
            self.unreachable.append("%s: log10 q = %.1f, too few bits for a reference value" % (name, lq))
            return False
        if t not in self:
            self.append(t)
            self.names.append(name)
        return True


def _ref_split(r, bias=3):
    """r REF reads, nearly balanced over the strands."""
    return (r + 1) // 2 + bias, r // 2 - bias


def _nearest(tables, target):
    return min(tables, key=lambda t: abs(log10_q(t) - target))


def _grid(lo, hi, points=160):
    """Integers from lo to hi, all of them when few, else geometrically spaced."""
    if hi - lo <= points:
        return list(range(lo, hi + 1))
    f = (hi / max(lo, 1)) ** (1.0 / points)
    out, x = {lo, hi}, float(max(lo, 1))
    while x < hi:
        out.add(int(x))
        x *= f
    return sorted(out)


@functools.lru_cache(maxsize=None)
def corpus(n_samples):
    """The tables of a row of n_samples (a Corpus, built once per row length and shared: leave it unchanged)."""
    N = int(n_samples)
    C = Corpus(N)
    maf = C.min_af

    def ref_for_candidate(a):
        """REF reads beside `a` ALT reads so that ALT stays well above min_af."""
        return max(2 * a, min(N - a, 400, int(0.8 * a / maf) - a))

    def ref_for_hom_ref(a):
        """REF reads beside `a` ALT reads so that ALT stays well below min_af."""
        return max(200, int(math.ceil(1.1 * a / maf)))

    # ---- row margins 11 | 12 | 13: the product form and the first margin past it, the small row ALT and REF
    for m in PRODUCT_MARGINS:
        F, V = _ref_split(ref_for_candidate(m), 10)
        for pos, j in (("imin", 0), ("imax", m), ("interior", 4)):
            C.add("margin%d alt row at %s" % (m, pos), (F, V, m - j, j))       # n11 - imin = n22
            C.add("margin%d ref row at %s" % (m, pos), (j, m - j, F, V) if pos != "imax" else (m, 0, F, V))
    C.add("product form, first table jmin = 5 (ALT row)", (300, 3, 8, 4))
    C.add("product form, first table jmin = 5 (REF row)", (8, 4, 300, 3))

    # ---- hom-ref sites: ALT below min_af.  R = 33 is the first to leave the one-lane walk
    for k, R in enumerate(LANE_R + (LANE_MAX_TABLES + 1,)):
        a = R - 1
        r = ref_for_hom_ref(a)
        j = a // 2
        F = r // 2
        want = ("first", "last", "middle")[k % 3]     # where the walk [F - j, F + a - j] meets a multiple of 11
        F += {"first": (j - F) % 11, "last": (j - a - F) % 11, "middle": (j + 5 - F) % 11}[want]
        C.add("hom-ref R=%d, multiple of 11 %s" % (R, want), (F, r - F, a - j, j))
    a = 12
    r = ref_for_hom_ref(a)
    F = r // 2
    C.add("hom-ref, multiple of 11 at the first table", (F + (6 - F) % 11, r - F - (6 - F) % 11, 6, 6))
    C.add("hom-ref, multiple of 11 at the last table", (F + (-6 - F) % 11, r - F - (-6 - F) % 11, 6, 6))
    C.add("hom-ref, multiple of 11 in the middle", (F + (6 + 5 - F) % 11, r - F - (6 + 5 - F) % 11, 6, 6))
    C.add("hom-ref at imin, ALT all forward", (F, r - F, a, 0))
    C.add("hom-ref at imax, ALT all reverse", (F, r - F, 0, a))
    C.add("hom-ref, imin = 0", (3, r - 3, 2, 9))

    # ---- narrow: up to 128 tables, balanced and skewed
    for R in NARROW_R:
        a = R - 1
        r = ref_for_candidate(a)
        F, V = _ref_split(r)
        C.add("narrow R=%d balanced" % R, (F, V, (a + 1) // 2, a // 2))
        if R not in (16, 65, 128):
            continue
        cap = min(N - a, int(0.8 * a / maf) - a)
        fam = [(r2 // 2, r2 - r2 // 2, a - j, j) for r2 in (r,) for j in range(a // 2 + 1)]
        for r2 in _grid(2 * a, cap, 24):
            fam += [(r2 - V2, V2, 0, a) for V2 in _grid(a, r2 // 2)]
        fam += [(a, 0, 0, k2) for k2 in _grid(a, N - a)]   # ... or the REF row: every REF read on one strand, every ALT read on the other
        for key in ("q2", "q20", "q200"):
            t = _nearest(fam, SKEW_TARGET[key])
            if SKEWS[key][0] <= log10_q(t) <= SKEWS[key][1]:
                C.add("narrow R=%d %s" % (R, key), t)
            else:
                C.unreachable.append("narrow R=%d %s: nearest log10 q = %.1f" % (R, key, log10_q(t)))

    # ---- probed: more than 128 tables.  (d, K - d, K - d, W): all four margins >= K, R = K + 1, the observed table d
    # tables from imin; its mirror (K - d, d, W, K - d) sits d tables from imax.  W = d is the symmetric family, a larger
    # W moves the mode towards the observed table so that q stays a live number.
    def end_tables(K, d, live):
        W = d
        if live:
            W = max(d, min(N - 2 * K + d, K * K // max(d, 1) - 2 * K + d))
        return (d, K - d, K - d, W), (K - d, d, W, K - d)

    for R in PROBED_R:
        K = R - 1
        C.add("probed R=%d at the mode" % R, (K // 2, K - K // 2, K - K // 2, K // 2))
    for d in END_STEPS:
        for side, t in zip(("imin", "imax"), end_tables(128, d, False)):
            C.add("probed R=129, %d tables from %s" % (d, side), t)
    K_big = 999 if N >= 2 * 999 + 50 else 256
    for d in END_STEPS:
        for side, t in zip(("imin", "imax"), end_tables(K_big, d, True)):
            C.add("probed R=%d, %d tables from %s, mode beside it" % (K_big + 1, d, side), t)
    for R in (129, 257, 1000, N // 2 + 1):
        K = R - 1
        C.add("probed R=%d (0, k, k, 0)" % R, (0, K, K, 0))
        C.add("probed R=%d (k, 0, 0, k)" % R, (K, 0, 0, K))
    C.add("probed R~1000 at the mode", (499, 500, 500, 499))
    K = N // 2
    C.add("probed R=max at the mode", (K // 2, K - K // 2, K - K // 2, K // 2))
    sym = [(d, K - d, K - d, d) for d in range(K // 2 + 1)]
    for key in ("q2", "q20", "q200"):
        t = _nearest(sym, SKEW_TARGET[key])
        C.add("probed R=max %s, left of the mode" % key, t)
        C.add("probed R=max %s, right of the mode" % key, (t[1], t[0], t[3], t[2]))
    # q near 1e-300: a table of q * e^-60 is below the smallest double, which is where a probed tail ends.  The reference's
    # own walk multiplies an underflowed 0 until its next re-seed (n11 % 11 == 0) and, where the family is steep, loses
    # terms that matter at 1e-9: only tables on which its walk (serial_walk) is the exact rule's value to 5e-10 are used.
    deep = sorted((t for t in sym if SKEWS["q300"][0] <= log10_q(t) <= SKEWS["q300"][1]), key=lambda t: abs(log10_q(t) - SKEW_TARGET["q300"]))
    for side, mirror in (("left", False), ("right", True)):
        for t in deep[:8]:
            t = (t[1], t[0], t[3], t[2]) if mirror else t
            e = exact_two_sided(t)
            err = abs((decimal.Decimal(serial_walk(t)) - e) / e)
            if err < decimal.Decimal("5e-10"):
                C.add("probed R=max q300, %s of the mode" % side, t)
                break
            C.unreachable.append("probed R=max q300 %s: the reference's walk is %.0e off the exact rule" % (t, err))
        else:
            C.unreachable.append("probed R=max q300, %s of the mode: the reference's walk loses underflowed terms on every such table" % side)

    t = _nearest(sym, sum(Q150) / 2)
    C.add("probed R=max q150, left of the mode", t)
    C.add("probed R=max q150, right of the mode", (t[1], t[0], t[3], t[2]))
    # ---- steep ends: the family's first (or last) table below the double range, the observed table near the mode.  Row 1 holds
    # K reads, column 2 a few more than K, every other margin is large: ln p(imin) ~ -ln C(n, K) needs a few thousand reads.
    for R in STEEP_R:
        K = R - 1
        n_2 = K + 45
        y = max(1, (K * n_2 + N // 2) // N)       # row 1's reads in column 2, at the mode
        t = (K - y, y, N - n_2 - (K - y), n_2 - y)
        ln_end = _lbinom(N - K, n_2 - K) - _lbinom(N, n_2)    # ln p of the table with none of row 1's reads in column 1
        for end, tt in (("imin", t), ("imax", (t[1], t[0], t[3], t[2]))):
            if min(tt) >= 0 and ln_end < STEEP_LOG:
                C.add("steep end R=%d: ln p(%s) = %.0f beside an ordinary q" % (R, end, ln_end), tt)
            else:
                C.unreachable.append("steep end R=%d at %s: ln p there is %.0f with every read of the row, no underflow" % (R, end, ln_end))

    # ---- ties, the underflow band, SOR, degenerate margins
    for k in TIE_K:
        C.add("tie (k, k, k, k) k=%d" % k, (k, k, k, k))
        C.add("tie (k, 0, 0, k) k=%d" % k, (k, 0, 0, k))
    for k in UNDERFLOW_K:
        C.add("underflow band (k, 0, 0, k) k=%d" % k, (k, 0, 0, k))
    C.add("SOR: no REF read reverse", (300, 0, 20, 25))
    C.add("SOR: no ALT read forward", (300, 280, 0, 30))
    C.add("SOR: both cells empty", (300, 0, 0, 40))
    C.add("SOR: one-read cells", (300, 1, 1, 40))
    C.add("degenerate: ALT only", (0, 0, 50, 50))
    C.add("degenerate: one strand only", (50, 0, 50, 0))
    C.add("degenerate: REF only", (90, 90, 0, 0))
    C.add("degenerate: ALT only, one strand", (0, 0, 0, 70))
    C.add("degenerate: reverse strand only", (0, 70, 0, 70))
    C.add("q underflows to 0 at imin (0, k, k, 0) k=600", (0, 600, 600, 0))
    C.add("q underflows to 0 inside the family", (6, 594, 594, 6))

    # ---- a third base: the CVG table counts it, the VCF table only where it is called
    C.add("third base below min_af: VCF table margin 12, CVG table margin 13", (400, 380, 8, 4, 1, 0))
    C.add("third base called: one table for both", (300, 280, 40, 20, 30, 25))
    return C


# ------------------------------------------------------------------------------------------------ long rows
LONG_ROWS = (100000, 140000)   # the smallest round lengths that hold a product above 2^31 and a 65536 x 65536 wrap
MILLION = 1000000


def _walk_is_exact(t):
    """The rule of the q300 tables of corpus(): the reference's own walk is the exact rule's value to 5e-10."""
    e = exact_two_sided(t)
    return e > 0 and abs((decimal.Decimal(serial_walk(t)) - e) / e) < decimal.Decimal("5e-10")


def _add_wave_tables(C, exact_filter=True):
    """The wave-form targets of a long row, added to C: regimes, probe spans, round geometry, steep families with probes,
    the SOR products.  What the row length cannot hold goes to C.unreachable, by name."""
    N = C.n_samples
    # ---- R = 2, 63, 64 | 65, 255, 256 | 257: one table per lane, rounds, probes.  R - 1 ALT reads beside many REF reads is a row
    # margin of R - 1 (> 12 from R = 14 on); R = 2 takes a column margin of 1 so that no row margin is small
    C.add("wave R=2 (a column margin of 1)", (300, 1, 280, 0))
    for R in WAVE_R[1:]:
        a = R - 1
        C.add("wave R=%d at the mode" % R, (400, 394, (a + 1) // 2, a // 2))
    # ---- probe spans 62 | 63 | 64 on either side, q = 0 (the symmetric family) and q live (the mode beside the observed table)
    K = 999
    for d in WAVE_SPANS:
        for live in (False, True):
            W = max(d, min(N - 2 * K + d, K * K // d - 2 * K + d)) if live else d
            C.add("wave probed R=1000, %d tables from imin, %s" % (d, "q live" if live else "q = 0"), (d, K - d, K - d, W))
            C.add("wave probed R=1000, %d tables from imax, %s" % (d, "q live" if live else "q = 0"), (K - d, d, W, K - d))
    # ---- round geometry on whole families (65..256 tables: the window is the family): its length mod 64, the observed table's lane
    for R, d in ((128, 64), (129, 63), (191, 128), (255, 127), (256, 64), (193, 96)):
        K = R - 1
        C.add("wave rounds R=%d, observed table on lane %d" % (R, d % WAVE), (d, K - d, K - d + 300, d + 300))
    # ---- steep families with probes: row 1 holds K reads, small against N, column 2 two thousand more; the observed table at the
    # mode.  ln p(imin) ~ -ln C(N, K) is thousands of nats below the double range; a probe step is ~5 sigma of the family, so the
    # probes still leave a live first table (the model says so: below_floor is False on these)
    for R in WAVE_STEEP_R:
        K = R - 1
        n_2 = K + 2000
        y = max(1, (K * n_2 + N // 2) // N)
        t = (K - y, y, N - n_2 - (K - y), n_2 - y)
        for end, tt in (("imin", t), ("imax", (t[1], t[0], t[3], t[2]))):
            C.add("wave steep R=%d with probes, ln p(%s) below the double range, observed table at the mode" % (R, end), tt)
    # ---- a window of at least 100 rounds, and the shifted family whose window starts below the live floor after a probe: both
    # need a tiny live q inside the longest family; searched with the model over the symmetric family, kept where the
    # reference's own walk is the exact rule (as the q300 tables of corpus())
    K = N // 2
    for want, name in (("wave:rounds>=100", "a window of at least 100 rounds"),
                       ("wave:shifted_below_floor_after_probe", "shifted, first table below the live floor after a probe")):
        found = None
        lo_d = next(d for d in range(K // 2, 0, -1) if log10_q((d, K - d, K - d, d)) < -200.0)
        for d in range(lo_d, 0, -max(1, K // 20000)):
            t = (d, K - d, K - d, d)
            lq = log10_q(t)
            if lq < -300.0:
                break
            if want in wave_labels(t, classify_wave(t)) and (not exact_filter or _walk_is_exact(t)):
                found = t
                break
        if found is None:
            C.unreachable.append("wave %s: no table of the R=%d family with 1e-300 < q < 1e-200 has it" % (name, K + 1))
        else:
            C.add("wave %s, left of the mode" % name, found)
            C.add("wave %s, right of the mode" % name, (found[1], found[0], found[3], found[2]))
    # ---- SOR: products of two cells around 2^31 and 2^32 in the numerator (ref_fwd x alt_rev) and the denominator (ref_rev x alt_fwd)
    C.add("SOR den 46340 x 46341: below 2^31, no flag", (3, 46340, 46341, 5))
    C.add("SOR den 46341 x 46341: wraps negative", (3, 46341, 46341, 5))
    C.add("SOR num 46340 x 46341: below 2^31, no flag", (46340, 9, 11, 46341))
    C.add("SOR num 46341 x 46341: wraps negative", (46341, 9, 11, 46341))
    C.add("SOR den 65536 x 65536: wraps to 0", (1000, 65536, 65536, 1000))
    C.add("SOR num 65536 x 65536: wraps to 0", (65536, 9, 11, 65536))
    C.add("SOR den 65536 x 65536 wraps to 0 over a numerator of 0", (0, 65536, 65536, 0))
    C.add("SOR den 65537 x 65535: wraps to -1", (1000, 65537, 65535, 1000))
    C.add("SOR den 65537 x 65537: wraps to 131073", (1000, 65537, 65537, 1000))
    C.add("SOR: the CVG table overflows (46341 x 46341), the VCF table does not (46341 x 46340)", (3, 46341, 46340, 5, 1, 0))
    return C


@functools.lru_cache(maxsize=None)
def corpus_long(n_samples):
    """corpus(n_samples) plus the wave-form targets of a long row (a Corpus, built once and shared: leave it unchanged)."""
    base = corpus(n_samples)
    C = Corpus(int(n_samples))
    for name, t in zip(base.names, base):
        C.append(t)
        C.names.append(name)
    C.unreachable = list(base.unreachable)
    return _add_wave_tables(C)


@functools.lru_cache(maxsize=None)
def corpus_million():
    """At most 12 tables of 1,000,000 samples: the longest family at the mode and at q ~ 1e-200 on both sides, (k, 0, 0, k), a
    steep family with probes, 524288 x 8192 in SOR's denominator, and the shifted family whose window starts below the live
    floor after a probe (one probe step spans ~600 nats here).  The exact rule is too slow at this length: the tiny-q tables
    keep ln q above -520, where every term that matters to 1e-9 is a normal double in the reference's own walk."""
    N = MILLION
    C = Corpus(N)
    K = N // 2
    C.add("million R=max at the mode", (K // 2, K - K // 2, K - K // 2, K // 2))

    def sym(d):
        return (d, K - d, K - d, d)

    def first_d(pred):   # the largest d below the mode whose table satisfies pred (log10 q falls as d does)
        lo, hi = 1, K // 2
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if pred(sym(mid)):
                lo = mid
            else:
                hi = mid - 1
        return lo

    t = sym(first_d(lambda t: log10_q(t) <= -200.0))
    C.add("million R=max q200, left of the mode", t)
    C.add("million R=max q200, right of the mode", (t[1], t[0], t[3], t[2]))
    C.add("million (k, 0, 0, k) k=500000", (K, 0, 0, K))
    Ks, n_2 = 20000, 22000
    y = (Ks * n_2 + N // 2) // N
    C.add("million steep R=20001 with probes", (Ks - y, y, N - n_2 - (Ks - y), n_2 - y))
    C.add("million SOR den 524288 x 8192: wraps to 0", (1000, 524288, 8192, 1000))
    found = None
    for d in range(first_d(lambda t: log10_q(t) <= -205.0), 0, -25):
        t = sym(d)
        if log_p(t, d) < -520.0:
            break
        if "wave:shifted_below_floor_after_probe" in wave_labels(t, classify_wave(t)):
            found = t
            break
    if found is None:
        C.unreachable.append("million shifted, first table below the live floor after a probe: no table with -520 < ln q < -472")
    else:
        C.add("million shifted, first table below the live floor after a probe, left of the mode", found)
        # (the mirror's left span is the longer one: its probes leave a live first table, the same q on the other lanes)
        C.add("million, the mirror of that table", (found[1], found[0], found[3], found[2]))
    return C


def slab(tables, n_samples, order=None):
    """One site per (ref_fwd, ref_rev, alt_fwd, alt_rev[, other_fwd, other_rev]) table: ref A, alt C, a third base G for the
    optional pair (it makes the all-sites CVG table differ from the VCF one), every read at phred 30.  `order`: site i
    of the slab is table order[i] -- its reads, mapq and ranks move with it.  Cells past n_samples look covered.
    (The sites of test_gpu_parity._strand_table_slab, which stays with its two long-row tests.)"""
    S = len(tables)
    pitch = (n_samples + 15) // 16 * 16
    bs = np.zeros((S, pitch), np.uint8)
    q = np.full((S, pitch), 40, np.uint8)
    bs[:, :n_samples] = 8
    q[:, :n_samples] = 0
    for i, t in enumerate(tables):
        t = tuple(t) + (0, 0)
        cells = [0] * t[0] + [4] * t[1] + [1] * t[2] + [5] * t[3] + [2] * t[4] + [6] * t[5]
        assert len(cells) <= n_samples
        bs[i, :len(cells)] = cells
        q[i, :len(cells)] = 30
    rng = np.random.default_rng(5)
    mapq = np.full((S, pitch), 60, np.uint8)
    rpr = np.full((S, pitch), 7, np.uint16)
    mapq[:, :n_samples] = rng.integers(0, 61, (S, n_samples)).astype(np.uint8)
    rpr[:, :n_samples] = rng.integers(1, 151, (S, n_samples)).astype(np.uint16)
    out = {"n_sites": S, "n_samples": n_samples, "pitch": pitch, "base_strand": bs, "qual": q, "mapq": mapq, "rpr": rpr,
           "ref_base": np.zeros(S, np.uint8), "n_groups": 0}
    if order is not None:
        order = np.asarray(order)
        assert sorted(order.tolist()) == list(range(S))
        for k in ("base_strand", "qual", "mapq", "rpr"):
            out[k] = np.ascontiguousarray(out[k][order])
    return out


# ------------------------------------------------------------------------------------------------ sites that share a wave
WAVE_KINDS = ("product", "narrow", "probed", "degenerate", "q0")


def wave_kind(t, n_samples, maf):
    """(list, kind) of a site among the 16-lane solver's jobs: list 0 holds the candidates of at most two active bases,
    list 1 those of three or four; kind is the regime of the site's first Fisher test (its CVG table), `q0` where q
    underflows to 0 before a regime is entered.  None: the site is not solved by a 16-lane group."""
    t6 = tuple(t) + (0, 0)
    cv = (t6[0], t6[1], t6[2] + t6[4], t6[3] + t6[5])
    c = classify(cv, n_samples, maf, depths=(t6[0] + t6[1], t6[2] + t6[3], t6[4] + t6[5]))
    if c["solver"] != "g16":
        return None
    kind = c["regime"]
    if kind != "degenerate" and kind != "product" and c["log10q"] < ZERO_LOG10:
        kind = "q0"
    return (1 if c["n_active"] >= 3 else 0), kind


def wave_slots(kinds, order):
    """A MODEL of the job packing, not a record of what ran: candidates go four to a wave in site order, each list on its own.
    (The streaming kernel's waves append their candidates to the lists with one atomic add each and the fused kernel queues
    per workgroup, so the order across waves is not guaranteed; four orders make the mixes the model promises likely, and
    every order is held to the oracle whatever groups its sites met.)  Returns the
    (kind, slot) pairs and the ordered (kind in slot s, kind in slot s + 1) pairs of one wave that `order` produces."""
    slots, pairs = set(), set()
    count, prev = [0, 0], [None, None]
    for ti in order:
        k = kinds[ti]
        if k is None:
            continue
        lst, kind = k
        s = count[lst] % 4
        slots.add((kind, s))
        if s > 0:
            pairs.add((prev[lst], kind))
        prev[lst] = kind
        count[lst] += 1
    return slots, pairs


def wave_orders(tables, n_samples, maf, tries=96):
    """Four orders of the sites -- identity, reversed and two seeded permutations -- that between them put every kind into
    every group slot and every ordered pair of kinds into adjacent slots of one wave.  Returns (orders, slots, pairs)."""
    kinds = [wave_kind(t, n_samples, maf) for t in tables]
    S = len(tables)
    base = [np.arange(S), np.arange(S)[::-1].copy()]
    want_slots = {(k, s) for k in WAVE_KINDS for s in range(4)}
    want_pairs = {(a, b) for a in WAVE_KINDS for b in WAVE_KINDS}
    perms = [np.random.default_rng(1000 + s).permutation(S) for s in range(tries)]
    seen = [wave_slots(kinds, o) for o in base]
    ps = [wave_slots(kinds, p) for p in perms]
    best = None
    for a in range(tries):
        for b in range(a + 1, tries):
            slots = set().union(*(x[0] for x in seen), ps[a][0], ps[b][0])
            pairs = set().union(*(x[1] for x in seen), ps[a][1], ps[b][1])
            miss = len(want_slots - slots) + len(want_pairs - pairs)
            if best is None or miss < best[0]:
                best = (miss, a, b, slots, pairs)
            if miss == 0:
                break
        if best[0] == 0:
            break
    _, a, b, slots, pairs = best
    return base + [perms[a], perms[b]], slots, pairs


# ------------------------------------------------------------------------------------------------ the rule, twice
def serial_walk(t):
    """kt_fisher_exact's two-sided value of t the way htslib computes it (kfunc.c), in Python's doubles: every table's
    probability by the multiplicative step from the one before, re-seeded from lgamma where n11 % 11 == 0 or n22 == 0."""
    n11, n12, n21, n22 = t
    imin, imax, n1_, n_1, n = family(t)
    if imin == imax:
        return 1.0

    def lb(a, b):
        return 0.0 if b == 0 or a == b else math.lgamma(a + 1) - math.lgamma(b + 1) - math.lgamma(a - b + 1)

    def seed(i):
        return math.exp(lb(n1_, i) + lb(n - n1_, n_1 - i) - lb(n, n_1))

    state = [n11, seed(n11)]
    q = state[1]
    if q == 0.0:
        return 0.0

    def move(i):
        k, p = state
        if i % 11 and i + n - n1_ - n_1:
            if i == k + 1:
                state[:] = [i, p * ((n1_ - k) / i * (n_1 - k) / (i + n - n1_ - n_1))]
                return state[1]
            if i == k - 1:
                state[:] = [i, p * (k / (n1_ - i) * (k + n - n1_ - n_1) / (n_1 - i))]
                return state[1]
        state[:] = [i, seed(i)]
        return state[1]

    p, left, i = move(imin), 0.0, imin + 1
    while p < 0.99999999 * q and i <= imax:
        left += p
        p = move(i)
        i += 1
    if p < 1.00000001 * q:
        left += p
    p, right, j = move(imax), 0.0, imax - 1
    while p < 0.99999999 * q and j >= 0:
        right += p
        p = move(j)
        j -= 1
    if p < 1.00000001 * q:
        right += p
    return min(1.0, left + right)


def exact_two_sided(t):
    """_exact_two_sided, computed once per family and observed table: swapping the columns reverses the family and leaves the
    two-sided sum as it is, so a table and its mirror (n12, n11, n22, n21) share one value."""
    t = tuple(int(x) for x in t)
    return _exact_two_sided(min(t, (t[1], t[0], t[3], t[2])))


@functools.lru_cache(maxsize=None)
def _exact_two_sided(t):
    """kt_fisher_exact's two-sided value of t = (n11, n12, n21, n22) in 60-digit decimal arithmetic: every table's weight from
    the one before by the exact ratio, the weights normalised by their sum (Vandermonde: the family's probabilities sum to 1; the
    binomials of 100,000 reads as integers of 40,000 digits cost ten times the walk), the walk from either end up to the first table of
    at least 0.99999999 q, which is added when it is below 1.00000001 q (the doubles of those two literals)."""
    imin, imax, n1_, n_1, n = family(t)
    if imin == imax:
        return decimal.Decimal(1)
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ctx.Emin, ctx.Emax = -10 ** 9, 10 ** 9
        D = decimal.Decimal
        p = D(1)
        P = [p]
        n22 = imin + n - n1_ - n_1
        for i in range(imin, imax):
            p = p * ((n1_ - i) * (n_1 - i)) / ((i + 1) * (n22 + (i - imin) + 1))
            P.append(p)
        total = sum(P)
        P = [p / total for p in P]
        q = P[t[0] - imin]
        lo, hi = D(0.99999999) * q, D(1.00000001) * q
        i = 0
        left = D(0)
        while P[i] < lo and i + 1 < len(P):
            left += P[i]
            i += 1
        if P[i] < hi:
            left += P[i]
        j = len(P) - 1
        right = D(0)
        while P[j] < lo and j - 1 >= 0:
            right += P[j]
            j -= 1
        if P[j] < hi:
            right += P[j]
        return min(D(1), left + right)
