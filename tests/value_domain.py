"""Seeded slabs whose mapq, phred and read-position-rank planes reach the edges of the domains the ABI accepts (test helper,
not a conftest).

basevar_amd.synth.make_slab draws mapq 10..60, phred 2..41 and ranks 1..100; the kernels branch on the values beyond:
the pass-2 rank-sum tallies glue class, mapq and rank bytes into one word whose "< 0x200" compare is both the predicate and
the histogram index, and send a row holding a rank >= 256 to the window sweeps; the group histograms skip phred 64..127
when no cell of a row has bit 6 or 7; the tagged layout keeps a rank in 13 bits beside the call (a covered A-forward read of
rank 0 is the word 0x0000); the per-site tallies of tile jobs keep ranks below a window and pool the others.

edge_slab() starts from make_slab (whose draws stay as they are: test_oracle_cpu pins their digest) and writes the values
below on covered REF and ALT reads of the variant-class sites.  dense_slab() builds deep rows for the dominant-value tally
(bv_lds_add16_dom).  assert_edges_hit() makes a fixture that never reaches the edges fail instead of pass quietly."""
import numpy as np

from basevar_amd.synth import make_slab

MAPQ_EDGES = (0, 1, 59, 60, 61, 99, 100, 127, 128, 129, 200, 254, 255)
PHRED_EDGES = (0, 1, 2, 41, 42, 63, 64, 65, 92, 93)
RANK_EDGES = (0, 1, 254, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 16384, 32767, 32768, 65534, 65535)
# the largest rank of a variant-class row cycles through these: 255 keeps the row on the 256-rank perm form, 1023 fills the
# first window of the sweeps exactly, 8191 is the tagged layout's largest rank
ROW_RANK_CAPS = (255, 1023, 8191, 65535)
# site classes (AF of the first and second ALT base), cycled by site index: three sites in four carry ALT reads
EDGE_CLASSES = [(0.0, 0.0), (0.35, 0.0), (0.25, 0.15), (0.45, 0.0)]
DENSE_CLASSES = [(0.35, 0.0), (0.45, 0.0), (0.25, 0.15)]
# kinds of dense rows, cycled by site index: the mapq that most REF and ALT reads carry
DOM_60, DOM_0, DOM_255, DOM_UNLUCKY, DOM_SPLIT = range(5)


def read_classes(slab):
    """(REF reads, reads of a base other than REF) [S][N]: covered cells whose base is / is not the site's reference base."""
    N = int(slab["n_samples"])
    bs = np.asarray(slab["base_strand"])[:, :N]
    called = bs < 8
    ref = np.asarray(slab["ref_base"])[:, None]
    return called & ((bs & 3) == ref), called & ((bs & 3) != ref)


def _spread(plane, row, cells, values, per_value, rng, first=None):
    """Writes `values` (shuffled; `first` ahead of them) on up to per_value * len(values) of `cells` (sample indices)."""
    if cells.size == 0:
        return
    vals = list(rng.permutation(np.asarray(values)))
    if first is not None:
        vals.remove(first)
        vals.insert(0, first)
    cells = rng.permutation(cells)
    k = min(cells.size, per_value * len(vals))
    plane[row, cells[:k]] = np.tile(np.asarray(vals, dtype=plane.dtype), per_value)[:k]


def edge_slab(n_sites, n_samples, seed, coverage=0.2, n_groups=0, max_rank=65535, per_value=2, indel_frac=0.005,
              class_af=None):
    """make_slab(...) with the edge values on covered REF and ALT reads of every variant-class site: per site and read class
    (REF, ALT), every value of MAPQ_EDGES, PHRED_EDGES and the row's rank values on up to `per_value` reads each (cells
    chosen independently per plane).  The row's rank values are RANK_EDGES up to its cap (ROW_RANK_CAPS up to max_rank,
    cycled every four sites); the cap itself sits on a REF read, so the row's largest rank is exactly the cap.  With
    max_rank = 8191 every rank fits the tagged layout (synth.tag_ranks)."""
    classes = class_af if class_af is not None else EDGE_CLASSES
    slab = make_slab(n_sites, n_samples, seed=seed, coverage=coverage, n_groups=n_groups, class_af=classes, indel_frac=indel_frac)
    rng = np.random.default_rng([seed, 0xED6E])
    caps = [c for c in ROW_RANK_CAPS if c <= max_rank]
    is_ref, is_alt = read_classes(slab)
    for r in range(n_sites):
        if classes[r % len(classes)] == (0.0, 0.0):
            continue
        cap = caps[(r // len(classes)) % len(caps)]
        ranks = [v for v in RANK_EDGES if v <= cap]
        for cls, first in ((is_ref[r], cap), (is_alt[r], None)):
            cells = np.nonzero(cls)[0]
            _spread(slab["mapq"], r, cells, MAPQ_EDGES, per_value, rng)
            _spread(slab["qual"], r, cells, PHRED_EDGES, per_value, rng)
            _spread(slab["rpr"], r, cells, ranks, per_value, rng, first)
    return slab


def dense_slab(n_sites, n_samples, seed, per_value=2):
    """Deep rows (coverage 0.6 .. 1.0, every site of a variant class, no pop-groups): an eighth or more of every row's cells
    are REF / ALT reads, the rows whose rank-sum mapq tally counts a dominant value (bv_lds_add16_dom).  Row kinds, cycled:
      DOM_60, DOM_0, DOM_255  nine REF / ALT reads in ten carry mapq 60 / 0 / 255, the others MAPQ_EDGES;
      DOM_UNLUCKY             mapq 60 everywhere but on the first REF / ALT read of every block of samples, which holds a
                              value found nowhere else in the row -- the first passing lane of a slot names a value no other
                              lane holds;
      DOM_SPLIT               REF reads mapq 60, ALT reads mapq 255.
    Phred takes PHRED_EDGES and rank the edges up to 255 (the perm form, where the dominant-value tally lives) on up to
    `per_value` reads per value and class."""
    slab = make_slab(n_sites, n_samples, seed=seed, coverage=1.0, class_af=DENSE_CLASSES)
    rng = np.random.default_rng([seed, 0xD0D])
    N = n_samples
    for r in range(n_sites):  # coverage 0.6 .. 1.0 per row: uncovered cells get the batchfile's placeholders
        cov = 0.6 + 0.1 * (r % 5)
        drop = np.nonzero(rng.random(N) >= cov)[0]
        slab["base_strand"][r, drop] = 8
        for k in ("qual", "mapq", "rpr"):
            slab[k][r, drop] = 0
    is_ref, is_alt = read_classes(slab)
    ranks = [v for v in RANK_EDGES if v <= 255]
    block = max(64, (-(-N // 200) + 63) // 64 * 64)  # at most ~200 blocks: distinct values for every block's first read
    for r in range(n_sites):
        kind = r % 5
        ra = np.nonzero(is_ref[r] | is_alt[r])[0]
        mq = slab["mapq"]
        if kind in (DOM_60, DOM_0, DOM_255):
            mq[r, ra] = (60, 0, 255)[kind]
            other = ra[rng.random(ra.size) < 0.1]
            mq[r, other] = rng.choice(np.asarray(MAPQ_EDGES, np.uint8), size=other.size)
        elif kind == DOM_UNLUCKY:
            mq[r, ra] = 60
            firsts = np.unique(np.searchsorted(ra, np.arange(0, N, block)))
            firsts = ra[firsts[firsts < ra.size]]
            pool = np.array([v for v in range(256) if v != 60], np.uint8)
            mq[r, firsts] = rng.permutation(pool)[:firsts.size]
        else:
            mq[r, np.nonzero(is_ref[r])[0]] = 60
            mq[r, np.nonzero(is_alt[r])[0]] = 255
        for cls in (is_ref[r], is_alt[r]):
            cells = np.nonzero(cls)[0]
            _spread(slab["qual"], r, cells, PHRED_EDGES, per_value, rng)
            _spread(slab["rpr"], r, cells, ranks, per_value, rng)
    return slab


def ranksum_sites(records):
    """Indices of the sites that came back VARIANT with their rank sums formed (BV_SITE_VARIANT | BV_SITE_RANKSUM)."""
    st = getattr(records, "sites", records)["status"]
    return np.nonzero((st & 0x12) == 0x12)[0]


def assert_edges_hit(slab, records, max_rank=65535, mapq=MAPQ_EDGES, phred=PHRED_EDGES):
    """Every edge value (ranks: those up to max_rank) sits on a REF read AND on an ALT read (a read of one of the site's
    ALT bases) of some site that `records` call VARIANT with BV_SITE_RANKSUM set.  `slab` holds plain ranks."""
    rec = getattr(records, "sites", records)
    v = ranksum_sites(rec)
    assert v.size, "no variant site with rank sums"
    N = int(slab["n_samples"])
    bs = np.asarray(slab["base_strand"])[v, :N]
    is_ref, _ = read_classes({"base_strand": bs, "ref_base": np.asarray(slab["ref_base"])[v], "n_samples": N})
    alt_mask = np.zeros((v.size, 4), bool)
    for k in range(4):
        has = rec["n_alt"][v] > k
        alt_mask[np.nonzero(has)[0], rec["alt"][v, k][has] & 3] = True
    is_alt = (bs < 8) & np.take_along_axis(alt_mask, (bs & 3).astype(np.int64), axis=1)
    ranks = [x for x in RANK_EDGES if x <= max_rank]
    for name, want in (("mapq", mapq), ("qual", phred), ("rpr", ranks)):
        pl = np.asarray(slab[name])[v, :N]
        for cls, cname in ((is_ref, "REF"), (is_alt, "ALT")):
            seen = set(np.unique(pl[cls]).tolist())
            miss = [x for x in want if x not in seen]
            assert not miss, "%s values %s sit on no %s read of a variant site with rank sums" % (name, miss, cname)
