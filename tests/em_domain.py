"""Seeded slabs whose sites are built so that the EM loop's stopping rule decides something (test helper, not a conftest).

The reference's EM (src/algorithm.h:210-255) sums abs(llh_new - llh_old) over the samples, and that abs is int abs(int): a
pass adds to the sum only for samples whose log-marginal moved by 1 or more, and the loop stops after the first pass in which
none did (or after 100).  The slabs of value_domain.py and allele_domain.py almost never loop twice.  Here every site is
searched, with a serial float64 MODEL of the reference's EM and LRT on (base, phred, count) classes of reads (em_model,
lrt_model: written from algorithm.h and basetype.cpp, the reference's expressions in the reference's order, not from the
kernels), for a chosen number of loop passes, a chosen place of the loop in the LRT, and a chosen first-pass move of a
class's log-marginal beside the truncation step: see TAGS.  A tag whose search comes back empty raises.

A site holds up to four KINDS of reads: "main" (some hundred reads, phred >= 4 -- the width of its phred range sets the
site's bin class), "mix" (k_hi strong reads at phred 40 and up and k_lo weak ones at phred 1..3 of ONE base: the first
m-step hands the weak reads to the other bases, the base's frequency falls by about k_hi / (k_hi + k_lo) and the marginal
of its strong reads with it -- the SHRINKING side), "third" and "fourth" (some tens of strong reads).  The GROWING side is a
subset that leaves out the site's largest base: its start frequencies sum to the share s of the reads it holds, the first
m-step rescales them to 1, and every marginal grows by about 1 / s; s either side of 1/e brackets the step.  Phreds are
laid out cyclically over a kind's range, so what the model says of a recipe does not depend on the seed; the seed permutes
the bases, picks among a tag's candidates and draws cells, strands, mapq and ranks.

With pop-groups three groups take a fixed fraction of every kind (so that their own lrt([REF] + alts) loops as the site's
does), the third of them at most SMALL_GROUP samples; further groups hold reads of the main base only."""
import itertools

import numpy as np

import basevar_amd
from allele_domain import MARGIN_REL, _empty_slab, _margin_ok

MLN10TO10 = -0.23025850929940458  # src/basetype.h
LRT_THRESHOLD = 24.0
INV_E = 0.36787944117144233
SMALL_GROUP = 48
SHARES = (0.30, 0.20, 0.12)  # what the first three pop-groups take of every kind of read
BIN_BOUNDS = {"bins_few": (2, 16), "bins_l8": (17, 32), "bins_g48": (33, 48), "bins_g128": (49, 128), "bins_wave": (129, 400)}

# tag -> what a site declared with it shows (model_tags)
TAGS = (
    "passes_1", "passes_2", "passes_3", "passes_4", "passes_5plus",  # the site's LONGEST EM run takes that many loop passes
    "top_multi",  # the EM over the full active set loops twice or more
    "sub_3to2", "sub_4to3",  # so does a subset EM one level down
    "two_base",  # so does the top EM of a site with two active bases
    "single_1", "single_2",  # a single-base subset with depth / total just above / just below 1/e: 1 and 2 passes
    "ref_kept_multi", "ref_dropped_multi", "ref_N_multi",  # a multi-pass run, REF kept / dropped by the LRT / N
    "shrink_sliver", "shrink_one", "shrink_two", "inside",  # first-pass llh_new - llh_old of a class in (-1, -0.9943),
    "grow_sliver", "grow_one", "grow_two",  # (-1.01, -1], <= -2, |.| in (0.05, 0.9); (0.9943, 1), [1, 1.01), >= 2
    "big_count",  # a class of BIG_COUNT reads or more moves by 1 or more: delta = c * 1
    "bins_few", "bins_l8", "bins_g48", "bins_g128", "bins_wave",  # a multi-pass site of that many (base, phred) bins
    "q0",  # a site of three passes and more (<= 64 covered samples: two) with one phred-0 read: the generic EM body
    "ordered",  # a multi-pass site of <= 64 covered samples in a slab of longer rows: the per-sample replay
)
# rows of <= 64 samples hold at most 44 reads a site: no site of more than 48 bins
_FALL = "a run of k passes needs the mixed base to fall by e^(k-1): more reads than such a row holds"
OUT_OF_REACH_SHORT = {"passes_3": _FALL, "passes_4": _FALL, "passes_5plus": _FALL,
                      "shrink_two": "a fall by e^2 in one pass needs 0.78 k_lo / total < e^-2 with k_lo >= 7: 49 reads and more",
                      "bins_g128": "a row of <= 64 samples holds fewer reads than the class has bins",
                      "bins_wave": "a row of <= 64 samples holds fewer reads than the class has bins",
                      "ordered": "every site of such a row is replayed per sample: the other tags are this one"}
GROUP_TAGS = ("group_bins16", "group_bins64", "group_bins_more", "group_small")
SLIVER = 0.9943  # -log(0.37) = 0.99425, log(2.7) = 0.99325: beyond it a bin-based body takes the logarithm


def big_count(shallow):
    return 10 if shallow else 100


# ------------------------------------------------------------------ the model
def int_abs(d):
    """abs((int)d) as algorithm.h:245 compiles: NaN and out-of-range differences become INT_MIN, whose abs is itself."""
    d = np.asarray(d, np.float64)
    out = np.full(d.shape, -2147483648.0)
    ok = np.isfinite(d) & (np.abs(d) < 2147483648.0)
    out[ok] = np.abs(np.trunc(d[ok]))
    return out


def likelihoods(base, phred):
    """basetype.cpp:47-63: one row of four per class."""
    eps = np.exp(np.asarray(phred, np.float64) * MLN10TO10)
    lh = np.repeat((eps / 3)[:, None], 4, axis=1)
    lh[np.arange(len(eps)), np.asarray(base, np.int64)] = 1.0 - eps
    return lh


def em_model(lh, cnt, f):
    """EM (algorithm.h:210-255) on classes of `cnt` equal samples each.  Returns (the classes' llh_new - llh_old of every
    loop pass, final frequencies, sum of the log-marginals)."""
    cnt = np.asarray(cnt, np.float64)
    n = cnt.sum()
    f = np.asarray(f, np.float64)

    def e_step(f):  # :148-175
        L = lh * f
        marg = ((L[:, 0] + L[:, 1]) + L[:, 2]) + L[:, 3]
        with np.errstate(invalid="ignore", divide="ignore"):
            return L / marg[:, None], marg

    def m_step(post):  # :184-198
        return (post * cnt[:, None]).sum(axis=0) / n

    with np.errstate(invalid="ignore", divide="ignore"):
        post, marg = e_step(f)
        llh = np.log(marg)
        f = m_step(post)
        passes = []
        for _ in range(100):
            post, marg = e_step(f)
            f = m_step(post)
            new = np.log(marg)
            d = new - llh
            llh = new
            passes.append(d)
            if (cnt * int_abs(d)).sum() < 0.001:
                break
        f = m_step(post)
    return passes, f, float((cnt * llh).sum())


def lrt_model(base, phred, cnt, ref, min_af, specific=(0, 1, 2, 3)):
    """BaseType::lrt (basetype.cpp:130-199) on classes.  Returns a dict: runs -- one entry per EM run, in the reference's
    order, with the active set's size at that level (m), the subset and the per-pass differences; n_em, em_iters, the
    ALT tuple, whether REF was among the active bases and was dropped, and `trunc`: the smallest distance to an integer
    of any difference beyond 0.99 in size."""
    base = np.asarray(base, np.int64)
    cnt = np.asarray(cnt, np.int64)
    lh = likelihoods(base, phred)
    depth = np.array([cnt[base == b].sum() for b in range(4)], np.float64)
    total = float(cnt.sum())
    out = dict(runs=[], alt=(), n_em=0, em_iters=0, trunc=np.inf, active0=(), kept=())
    if total == 0:
        return out
    active = [b for b in specific if b < 4 and depth[b] / total >= min_af]
    out["active0"] = tuple(active)
    if not active:
        return out

    def F(bases, n):
        res = []
        for sub in itertools.combinations(bases, n):
            f0 = np.zeros(4)
            for b in sub:
                f0[b] = depth[b] / total
            passes, f, lr = em_model(lh, cnt, f0)
            out["runs"].append(dict(m=len(bases), subset=sub, passes=passes))
            for d in passes:
                a = np.abs(d[np.isfinite(d)])
                a = a[a > 0.99]
                if a.size:
                    out["trunc"] = min(out["trunc"], float(np.abs(a - np.rint(a)).min()))
            res.append((sub, f, lr))
        return res

    var = F(active, len(active))
    freq, lr_alt = var[0][1], var[0][2]
    for n in range(len(active) - 1, 0, -1):  # the bound is the ORIGINAL size, :151
        var = F(active, n)
        chiv = [2 * (lr_alt - v[2]) for v in var]
        i_min = 0
        for j in range(len(chiv)):
            if chiv[j] < chiv[i_min]:
                i_min = j
        lr_alt = var[i_min][2]
        if chiv[i_min] < LRT_THRESHOLD:
            active, freq = list(var[i_min][0]), var[i_min][1]
        else:
            break
    out["kept"] = tuple(active)
    out["alt"] = tuple(b for b in active if b != ref)
    out["n_em"] = len(out["runs"])
    out["em_iters"] = sum(len(r["passes"]) for r in out["runs"])
    return out


def site_classes(slab, s, members=None):
    """(base, phred, count) classes of site s (of the samples `members`, a boolean mask)."""
    N = int(slab["n_samples"])
    bs = np.asarray(slab["base_strand"])[s, :N]
    c = bs < 8
    if members is not None:
        c = c & members
    key = (bs[c] & 3).astype(np.int64) * 256 + np.asarray(slab["qual"])[s, :N][c]
    u, k = np.unique(key, return_counts=True)
    return u >> 8, u & 255, k


def model_tags(R, ref, n_bins, covered, shallow, has_q0=False):
    """The tags of TAGS that a site with the model's result R shows."""
    tags = set()
    runs = R["runs"]
    if len(R["active0"]) < 2:
        return tags
    longest = max(len(r["passes"]) for r in runs)
    tags.add("passes_%d" % longest if longest < 5 else "passes_5plus")
    multi = longest >= 2
    top = runs[0]
    if len(top["passes"]) >= 2:
        tags.add("top_multi")
        if len(top["subset"]) == 2:
            tags.add("two_base")
    for r in runs[1:]:
        k, m, p = len(r["subset"]), r["m"], len(r["passes"])
        if p >= 2 and m == 3 and k == 2:
            tags.add("sub_3to2")
        if p >= 2 and m == 4 and k == 3:
            tags.add("sub_4to3")
        if k == 1 and not has_q0:
            d = float(r["passes"][0][0])  # -log(f_init), the same for every class
            if p == 1 and 0.9 < d < 1.0:
                tags.add("single_1")
            if p == 2 and 1.0 <= d < 1.03:
                tags.add("single_2")
    if multi:
        if ref > 3:
            tags.add("ref_N_multi")
        elif ref in R["kept"]:
            tags.add("ref_kept_multi")
        elif ref in R["active0"]:
            tags.add("ref_dropped_multi")
        for t, (lo, hi) in BIN_BOUNDS.items():
            if lo <= n_bins <= hi:
                tags.add(t)
        if has_q0 and longest >= (2 if covered <= 64 else 3):  # three passes: a generic body that stops after two shows
            tags.add("q0")
        if covered <= 64 and not shallow:
            tags.add("ordered")
    for r in runs:
        if len(r["subset"]) < 2:
            continue  # the bin-based bodies run subsets of two bases and more
        d = r["passes"][0]
        d = d[np.isfinite(d)]
        if ((d > -1.0) & (d < -SLIVER)).any(): tags.add("shrink_sliver")
        if ((d <= -1.0) & (d > -1.01)).any(): tags.add("shrink_one")
        if (d <= -2.0).any(): tags.add("shrink_two")
        if ((d > SLIVER) & (d < 1.0)).any(): tags.add("grow_sliver")
        if ((d >= 1.0) & (d < 1.01)).any(): tags.add("grow_one")
        if (d >= 2.0).any(): tags.add("grow_two")
        if multi and ((np.abs(d) > 0.05) & (np.abs(d) < 0.9)).any(): tags.add("inside")
        for dd in r["passes"]:
            if ((r["cnt"] >= big_count(covered <= 64)) & (int_abs(dd) >= 1)).any(): tags.add("big_count")
    return tags


# ------------------------------------------------------------------ recipes
# a recipe: ((role, lo, hi, count), ...) with roles main, mix_hi, mix_lo, third, fourth; refrole main / mix / N; q0
def _layout(lo, hi, count):
    """`count` phreds laid cyclically over lo..hi."""
    return (lo + np.arange(count) % (hi - lo + 1)).astype(np.uint8)


def _recipe_classes(recipe):
    base, phred = [], []
    bases = {"main": 0, "mix_hi": 1, "mix_lo": 1, "third": 2, "fourth": 3}
    for role, lo, hi, count in recipe["kinds"]:
        base.append(np.full(count, bases[role])); phred.append(_layout(lo, hi, count))
    base, phred = np.concatenate(base), np.concatenate(phred).astype(np.int64)
    if recipe.get("q0"):
        phred[0] = 0  # the first main read
    u, k = np.unique(base * 256 + phred, return_counts=True)
    return u >> 8, u & 255, k


def _evaluate(recipe, min_af, shallow):
    b, q, c = _recipe_classes(recipe)
    ref = {"main": 0, "mix": 1, "N": 4}[recipe["ref"]]
    R = lrt_model(b, q, c, ref, min_af)
    for r in R["runs"]:
        r["cnt"] = c
    covered = int(c.sum())
    return R, model_tags(R, ref, len(c), covered, shallow, has_q0=bool(recipe.get("q0")))


def _shrink_recipes(shallow):
    """The strong-plus-weak ALT beside a strong main base, with and without a third and a fourth base."""
    mlo, mhi = (35, 36)
    if shallow:  # no third base: main reads, strong reads, weak reads and their phreds over a finer grid
        for main in (16, 18, 20, 22, 24, 26, 28, 30, 32):
            for k_hi in (1, 2, 3, 4):
                for k_lo in range(2, 24):
                    if main + k_hi + k_lo > 44:
                        continue
                    for wlo, whi in ((1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)):
                        yield dict(kinds=(("main", mlo, mhi, main), ("mix_hi", 40, 40, k_hi), ("mix_lo", wlo, whi, k_lo)), ref="main")
    else:
        # the longest runs: one strong read, and weak phred-1 reads that leave the base by a factor just below 1/e a pass
        # (a phred-1 read's posterior is about 0.78 f / f_main: 0.78 k_lo / total just below 1/e), down to the floor of one read
        for k_lo in (150, 200, 300):
            for y in (1.2, 1.3, 1.4, 1.5, 1.6, 1.8):
                yield dict(kinds=(("main", mlo, mhi, int(k_lo * y)), ("mix_hi", 40, 40, 1), ("mix_lo", 1, 1, k_lo)), ref="main")
        # a run of k passes needs k - 1 falls by e or more after the one the pre-loop step takes: k_lo + 1 >= e^k.  Five
        # passes take some 1,300 reads (so rows of 1,500 samples hold such a site only where most samples are in no extra group)
        for k_lo, main in ((500, 760), (500, 780), (500, 800), (550, 830)):
            yield dict(kinds=(("main", mlo, mhi, main), ("mix_hi", 40, 40, 1), ("mix_lo", 1, 1, k_lo)), ref="main")
    main = 30 if shallow else 300
    grid_hi = (1, 2, 3) if shallow else (1, 2, 3, 5, 7, 20)
    for extra in (0, 1, 2):
        for k_hi in grid_hi:
            los = (2, 3, 4, 5, 6, 8, 10) if shallow else sorted({2, 3, 5, 6, 8, 12, 13, 19, 20, 35, 54, 60, 100, 150, int(1.7 * k_hi), int(1.72 * k_hi) + 1, 2 * k_hi})
            for k_lo in los:
                if k_lo < 2 or (shallow and main + k_hi + k_lo + 5 * extra > 44):
                    continue
                for wlo, whi in ((1, 1), (1, 3), (3, 3)):
                    kinds = [("main", mlo, mhi, main), ("mix_hi", 40, 40, k_hi), ("mix_lo", wlo, whi, k_lo)]
                    if extra >= 1:
                        kinds.append(("third", 38, 38, 5 if shallow else 30))
                    if extra >= 2:
                        kinds.append(("fourth", 37, 37, 4 if shallow else 25))
                    yield dict(kinds=tuple(kinds), ref="main")


def _grow_recipes(shallow):
    """Strong bases only; the largest holds 1 - s of the reads, s around 1/e and around e^-2."""
    totals = (38, 41, 43, 44) if shallow else (380, 400, 419, 433, 450)
    for T in totals:
        near = {int(T * INV_E) + d for d in (-1, 0, 1, 2)} | {int(T * 0.12), int(T * 0.30), int(T * 0.40)}
        for k in sorted(near):
            for parts in (2, 3):
                if k < 2 * parts + 1:
                    continue
                first = k // parts + parts
                rest = k - first
                sub = [first, rest] if parts == 2 else [first, rest - rest // 2 + 1, rest // 2 - 1]
                if len(set(sub)) < len(sub) or min(sub) < 1:
                    continue
                kinds = [("main", 35, 36, T - k)] + [(r, 40 - i, 40 - i, c) for i, (r, c) in enumerate(zip(("mix_hi", "third", "fourth"), sub))]
                yield dict(kinds=tuple(kinds), ref="main")
    # two strong bases with the smaller either side of 1/e: the single-base subsets
    for T in totals:
        for k in {int(T * INV_E) + d for d in (-1, 0, 1, 2)}:
            yield dict(kinds=(("main", 35, 36, T - k), ("mix_hi", 40, 40, k)), ref="main")


def _widen(recipe, tag):
    """The recipe with its main (and third) reads spread over as many phreds as the bin class asks."""
    lo, hi = {"bins_few": (35, 36), "bins_l8": (25, 40), "bins_g48": (10, 45), "bins_g128": (8, 93), "bins_wave": (4, 93)}[tag]
    kinds = []
    for role, klo, khi, count in recipe["kinds"]:
        if role == "main":
            kinds.append((role, lo, min(hi, lo + count - 1), count))
        elif role == "third" and tag == "bins_wave":
            kinds.append((role, 10, min(93, 10 + count + 14), count))
        elif role == "mix_hi" and tag == "bins_wave":
            kinds.append((role, 40, min(93, 40 + count - 1), count))
        else:
            kinds.append((role, klo, khi, count))
    return dict(recipe, kinds=tuple(kinds))


_catalogues = {}
PER_TAG = 6  # candidates kept per tag


def catalogue(shallow):
    """tag -> up to PER_TAG recipes that the model shows to carry it, every difference beyond 0.99 at MARGIN_REL or more from an
    integer.  Also "longest": the most loop passes any searched run took.  Searched once per process and regime, at the
    largest min_af (0.01) and with every base of a recipe active there, so that a smaller min_af changes nothing."""
    key = bool(shallow)
    if key in _catalogues:
        return _catalogues[key]
    cat = {t: [] for t in TAGS}
    longest = 0

    def offer(recipe, only=None, cap=PER_TAG):
        nonlocal longest
        R, tags = _evaluate(recipe, 0.01, shallow)
        n_bases = len({"mix" if k[0].startswith("mix") else k[0] for k in recipe["kinds"]})
        if len(R["active0"]) != n_bases or R["trunc"] < 10 * MARGIN_REL:
            return set(), R
        longest = max(longest, max(len(r["passes"]) for r in R["runs"]))
        for t in tags:
            if (only is None or t in only) and len(cat[t]) < cap and recipe not in cat[t]:
                cat[t].append(recipe)
        return tags, R

    plain = {t for t in TAGS if not t.startswith("bins_") and t not in ("q0", "ordered", "ref_dropped_multi", "ref_N_multi")} | {"bins_few"}
    variant, plainly = [], []  # multi-pass recipes that keep an ALT (their pop-groups are solved), and the others
    for r in itertools.chain(_grow_recipes(shallow), _shrink_recipes(shallow)):
        tags, R = offer(r, plain)
        if "top_multi" in tags and len(r["kinds"]) >= 3:
            (variant if R["alt"] else plainly).append(r)
    derived = ("ref_dropped_multi", "ref_N_multi", "q0", "bins_l8", "bins_g48", "bins_g128", "bins_wave")
    for pool, cap in ((variant[::2], PER_TAG // 2), (plainly[::3], PER_TAG), (variant, PER_TAG)):
        for r in pool:
            if all(len(cat[t]) >= cap for t in derived if not (shallow and t in OUT_OF_REACH_SHORT)):
                break
            for ref in ("mix", "N"):
                offer(dict(r, ref=ref), ("ref_dropped_multi", "ref_N_multi"), cap)
            offer(dict(r, q0=True), ("q0",), cap)
            for t in ("bins_l8", "bins_g48", "bins_g128", "bins_wave"):
                if not (shallow and t in OUT_OF_REACH_SHORT):
                    offer(_widen(r, t), (t,), cap)
    cat["longest"] = longest
    _catalogues[key] = cat
    return cat


# ------------------------------------------------------------------ the slab
class _Pools:
    """Samples of the three built pop-groups, of the further groups (reads of the main base only) and of no group."""

    def __init__(self, n, n_groups, rng):
        self.n, self.G = n, n_groups
        gid = np.full(n, 0xFF, np.uint8)
        order = rng.permutation(n)
        self.built, self.extra = [], []
        at = 0
        if n_groups:
            sizes = [int(0.30 * n), int(0.20 * n), min(SMALL_GROUP, max(1, n // 5))][:n_groups]
            for g, k in enumerate(sizes):
                self.built.append(order[at:at + k]); gid[order[at:at + k]] = g; at += k
            extra = n_groups - len(sizes)
            if extra > 0:
                each = max(1, int(0.25 * n) // extra)
                for k in range(extra):
                    self.extra.append(order[at:at + each]); gid[order[at:at + each]] = len(sizes) + k; at += each
        self.ungrouped = order[at:]
        self.group_id = gid


def _write_site(slab, s, rng, pools, recipe, perm):
    """Writes the recipe's reads to row s: role bases through `perm`; each built group takes SHARES of every kind, a run of
    neighbours in the kind's phred layout (at least one read of a kind of three or more)."""
    T = sum(k[3] for k in recipe["kinds"])
    role_base = {"main": perm[0], "mix_hi": perm[1], "mix_lo": perm[1], "third": perm[2], "fourth": perm[3]}
    free = [rng.permutation(g) for g in pools.built]
    used = [0] * len(free)
    rest = rng.permutation(pools.ungrouped)
    rest_at = 0
    shares = list(SHARES[:len(free)])
    if len(shares) == 3:
        shares[2] = min(shares[2], 44.0 / T, (free[2].size - 2.0) / T)
    first = True
    for role, lo, hi, count in recipe["kinds"]:
        phred = _layout(lo, hi, count)
        if first and recipe.get("q0"):
            phred[0] = 0
        first = False
        taken = np.zeros(count, bool)
        cells = np.zeros(count, np.int64)
        for g, share in enumerate(shares):
            left = np.nonzero(~taken)[0]
            k = int(round(share * count))
            if k == 0 and count >= 3 - g:
                k = 1
            k = min(k, left.size, free[g].size - used[g])
            if k <= 0:
                continue
            pick = left[:k]  # neighbours in the cyclic layout: min(k, width of the range) phreds
            cells[pick] = free[g][used[g]:used[g] + k]
            used[g] += k
            taken[pick] = True
        if role == "main":  # the further groups: a few reads of the main base each
            for g in pools.extra:
                left = np.nonzero(~taken)[0]
                if left.size <= max(8, count // 8):
                    break
                k = min(3, g.size)
                pick = left[:k]
                cells[pick] = rng.permutation(g)[:k]
                taken[pick] = True
        left = np.nonzero(~taken)[0]
        if rest_at + left.size > rest.size:
            raise RuntimeError("a site of %d reads does not fit beside the pop-groups of a row of %d samples" % (T, pools.n))
        cells[left] = rest[rest_at:rest_at + left.size]
        rest_at += left.size
        b = role_base[role]
        slab["base_strand"][s, cells] = b | (rng.integers(0, 2, count, dtype=np.uint8) << 2)
        slab["qual"][s, cells] = phred
        slab["mapq"][s, cells] = np.where(rng.random(count) < 0.8, 60, rng.integers(10, 60, count)).astype(np.uint8)
        slab["rpr"][s, cells] = rng.integers(1, 101, count).astype(np.uint16)
    N = int(slab["n_samples"])
    unused = np.nonzero(slab["base_strand"][s, :N] == 8)[0]
    k = min(2, unused.size)  # two indel cells, as make_slab's indel_frac leaves them
    slab["base_strand"][s, rng.permutation(unused)[:k]] = 9 + np.arange(k, dtype=np.uint8)
    slab["ref_base"][s] = {"main": perm[0], "mix": perm[1], "N": 4}[recipe["ref"]]


def _clear(slab, s):
    n = int(slab["n_samples"])
    slab["base_strand"][s, :n] = 8
    for k in ("qual", "mapq", "rpr"):
        slab[k][s, :n] = 0


def wanted_tags(n_samples, n_groups=0):
    """The classes a slab of that row length must show: all of TAGS but OUT_OF_REACH_SHORT on rows of <= 64 samples, and
    with three pop-groups or more GROUP_TAGS (on such short rows every group is a small one)."""
    out = [t for t in TAGS if not (n_samples <= 64 and t in OUT_OF_REACH_SHORT)]
    if n_groups >= 3:
        out += ["group_small"] if n_samples <= 64 else list(GROUP_TAGS)
    return out


def group_tag(bins, covered):
    return "group_small" if covered <= 64 else "group_bins16" if bins <= 16 else "group_bins64" if bins <= 64 else "group_bins_more"


# which site classes a pop-group class is searched among
GROUP_FROM = {"group_small": ("two_base", "sub_3to2"), "group_bins16": ("two_base", "sub_3to2", "bins_few"),
              "group_bins64": ("bins_g48", "bins_l8", "bins_g128"), "group_bins_more": ("bins_wave", "bins_g128")}


def em_slab(n_samples, seed, n_groups=0, per_tag=2, restatement=None):
    """(slab, declared).  declared: per site a dict -- want (the class it was searched for), tags (all it shows), n_em,
    em_iters and longest (the model's, on the cells of the slab), bins, covered, trunc (the smallest distance to an integer
    of a difference beyond 0.99, the site's pop-groups included), alt, and with pop-groups groups: {group: (bins, covered,
    loop passes of the group's longest run)} for the three built groups of a variant site, and group_tags.  The slab's own
    figures ride in declared[0]["slab"]: longest, the most loop passes of a run in the slab.  per_tag sites are built per
    class of wanted_tags().  With `restatement` (an oracle.Restatement or the fixture), a site whose oracle margin is
    below MARGIN_REL * max(1, |chi2|) gives way to the class's next candidate; a class with no candidate left raises."""
    n = int(n_samples)
    maf = float(basevar_amd.min_af(n))
    shallow_only = n <= 64
    cat = catalogue(shallow_only)
    plan = []
    for t in wanted_tags(n, n_groups):
        if t == "ordered":
            sh = catalogue(True)
            cands = sh["passes_2"][:3] + sh["sub_3to2"][:3]
        elif t in GROUP_TAGS:
            cands = [r for src in GROUP_FROM[t] for r in cat[src]]
        else:
            cands = list(cat[t])
        if not cands:
            raise RuntimeError("no site of class %s was found at %d samples" % (t, n))
        for k in range(min(per_tag, len(cands))):
            plan.append(dict(want=t, cands=cands, at=(seed + k) % len(cands), tried=0))
    S = len(plan)
    slab = _empty_slab(S, n)
    pools = _Pools(n, n_groups, np.random.default_rng([seed, n, 0xE301]))
    if n_groups:
        slab["n_groups"] = n_groups
        slab["group_id"] = pools.group_id
    declared = [None] * S

    def build(s):
        p = plan[s]
        while True:
            if p["tried"] >= len(p["cands"]):
                raise RuntimeError("no candidate of class %s keeps its margins at %d samples" % (p["want"], n))
            recipe = p["cands"][(p["at"] + p["tried"]) % len(p["cands"])]
            rng = np.random.default_rng([seed, n, s, p["tried"]])
            perm = [int(b) for b in rng.permutation(4)]
            _clear(slab, s)
            _write_site(slab, s, rng, pools, recipe, perm)
            d = describe_site(slab, s, maf, shallow_only)
            d["want"] = p["want"]
            if p["want"] in d["tags"] | d["group_tags"] and d["trunc"] >= MARGIN_REL:
                declared[s] = d
                return
            p["tried"] += 1

    for s in range(S):
        build(s)
    if restatement is not None:
        for _ in range(PER_TAG + 1):
            e, _, m = restatement.run_with_margins(slab, maf, n_threads=16)
            tight = [s for s in range(S) if not _margin_ok(m[s], e["chi2"][s])]
            if not tight:
                break
            for s in tight:
                plan[s]["tried"] += 1
                build(s)
        else:
            raise RuntimeError("sites %s keep an oracle margin below %g" % (tight, MARGIN_REL))
    declared[0]["slab"] = dict(longest=max(d["longest"] for d in declared), searched_longest=cat["longest"])
    return slab, declared


def describe_site(slab, s, maf, shallow):
    """What the model says of site s as it stands in the slab."""
    b, q, c = site_classes(slab, s)
    ref = int(slab["ref_base"][s])
    R = lrt_model(b, q, c, ref, maf)
    for r in R["runs"]:
        r["cnt"] = c
    covered = int(c.sum())
    tags = model_tags(R, ref, len(c), covered, shallow, has_q0=bool((q == 0).any()))
    d = dict(tags=tags, n_em=R["n_em"], em_iters=R["em_iters"], longest=max(len(r["passes"]) for r in R["runs"]), bins=len(c),
             covered=covered, trunc=R["trunc"], alt=R["alt"], groups={})
    G = int(slab.get("n_groups", 0))
    if G and R["alt"]:
        gid = np.asarray(slab["group_id"])[:int(slab["n_samples"])]
        for g in range(min(G, 3)):
            gb, gq, gc = site_classes(slab, s, gid == g)
            if gc.size == 0:
                continue
            GR = lrt_model(gb, gq, gc, ref, maf, specific=(ref,) + R["alt"])
            if GR["runs"]:
                d["groups"][g] = (len(gc), int(gc.sum()), max(len(r["passes"]) for r in GR["runs"]))
                d["trunc"] = min(d["trunc"], GR["trunc"])
    d["group_tags"] = {group_tag(bins, cov) for bins, cov, passes in d["groups"].values() if passes >= 2}
    return d


def assert_em_classes_hit(declared, records, n_samples, n_groups=0):
    """Reads the ORACLE's records: em_iters and n_em as the model declared them at every site, every wanted class present
    among the sites declared for it, every truncation margin MARGIN_REL or more, and with pop-groups every class of
    GROUP_TAGS that the row length can hold."""
    rec = getattr(records, "sites", records)
    assert len(rec) == len(declared)
    seen = set()
    for s, d in enumerate(declared):
        assert int(rec["em_iters"][s]) == d["em_iters"] and int(rec["n_em"][s]) == d["n_em"], \
            "site %d (%s): em_iters %d n_em %d, the model's %d %d" % (s, d["want"], rec["em_iters"][s], rec["n_em"][s], d["em_iters"], d["n_em"])
        assert d["want"] in d["tags"] | d["group_tags"] and d["trunc"] >= MARGIN_REL, "site %d (%s): tags %s, margin %g" % (s, d["want"], sorted(d["tags"]), d["trunc"])
        assert tuple(int(a) for a in rec["alt"][s][:rec["n_alt"][s]]) == d["alt"]
        seen.add(d["want"])
    miss = [t for t in wanted_tags(n_samples, n_groups) if t not in seen]
    assert not miss, "classes %s do not occur" % miss


def oracle_records(restatement, slab):
    """(records with the restatement's n_em, em_iters and chi2, group records, margins) of `slab`.  `restatement` is the
    fixture (the real reference's records where it is built) or a plain oracle.Restatement."""
    maf = basevar_amd.min_af(int(slab["n_samples"]))
    e, g, m = restatement.run_with_margins(slab, maf, n_threads=16)
    if getattr(restatement, "direct", False):  # neither count is observable through the reference: the restatement's
        import oracle
        r, _ = oracle.Restatement().run(slab, maf, n_threads=16)
        e = e.copy()
        e["n_em"] = r["n_em"]
        e["em_iters"] = r["em_iters"]
    return e, g, m


def assert_margins(margins, records):
    rec = getattr(records, "sites", records)
    bad = [(s, float(margins[s]), float(rec["chi2"][s])) for s in range(len(rec)) if not _margin_ok(margins[s], rec["chi2"][s])]
    assert not bad, "sites decided by a rounding-noise margin (site, margin, chi2): %s" % bad[:5]
