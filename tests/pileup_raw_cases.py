"""Raw runs of BAM records for the tests of the pileup's definition (bv_pileup_core.h) and of its device form (bv_pileup.hip): a
seeded campaign of valid rounds and hand-built cases with one purpose each.  Pure Python, no GPU code: the CPU tests
(test_pileup_core_cpu.py, under the sanitizers) and the GPU tests (test_gpu_pileup_raw.py) send the very same bytes.

A case is (runs, run_sample, n_samples, window, ref): the runs as bytes, the sample of each (non-decreasing), the number of
samples, the window (beg, end) inside one step of pr.REGION, and the reference's bases from its first on (bytes)."""
import functools

import numpy as np

import pileup_ref as pr
from pileup_ref import D, EQ, H, I, M, N, P, S, X

CAMPAIGN_SEEDS = list(range(1000, 1048))  # 48 rounds
SEED_BLOCKS = [CAMPAIGN_SEEDS[i:i + 8] for i in range(0, len(CAMPAIGN_SEEDS), 8)]
N_SAMPLES = [1, 2, 5, 63, 64, 65, 130]
WINDOW_ROWS = [1, 31, 32, 33, 64, 65, 1000]
MATCH_LEN = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 1000]
SKIP_LEN = [0, 1, 2, 5, 63, 64, 65, 129, 300]
QUERY_OPS = (M, I, S, EQ, X, P)  # P too: the host advances the query on P as on S, so a read holds bases for it
GB2 = pr.REGION[0] + pr.STEP      # the first row of the second step
FA = pr.reference()
_CODE = np.zeros(256, np.uint8)
for _i, _c in enumerate("=ACMGRSVTWYHKDBN"):
    _CODE[ord(_c)] = _i
_ACGTN = np.frombuffer(b"ACGTN", np.uint8)


def pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def make_read(rng, pos, cigar, tid=pr.TID, mapq=60, flag=0, qual=None, seq=None):
    """pr.read with seq and qual lengths derived from the CIGAR (P counted: see QUERY_OPS), letters of ACGTN, quals 0..255"""
    n = sum(ln for op, ln in cigar if op in QUERY_OPS)
    if seq is None:
        seq = _ACGTN[rng.integers(0, 5, n)].tobytes().decode()
    if qual is None:
        qual = rng.integers(0, 256, len(seq)).astype(np.uint8)
    return pr.read(rng, pos, cigar, tid=tid, mapq=mapq, flag=flag, seq=seq, qual=qual)


def pack(r):
    """pr.record_bytes, with numpy where that one loops over the bases (test_pileup_core_cpu.py holds the two equal)"""
    import struct
    name = r.get("name", "r").encode() + b"\0"
    code = _CODE[np.frombuffer(r["seq"].encode(), np.uint8)]
    if code.size & 1:
        code = np.append(code, np.uint8(0))
    packed = ((code[0::2] << 4) | code[1::2]).astype(np.uint8).tobytes()
    cig = np.array([(ln << 4) | op for op, ln in r["cigar"]], "<u4").tobytes()
    body = struct.pack("<iiBBHHHiiii", r["tid"], r["pos"], len(name), r["mapq"], 4680, len(r["cigar"]), r["flag"], len(r["seq"]), -1, -1, 0) + name + cig + packed + bytes(bytearray(r["qual"]))
    return struct.pack("<i", len(body)) + body


# ------------------------------------------------------------------------------------------------------------------ the campaign
def _body(rng):
    """1-4 matches of every kind with every other operation between them"""
    ops = []
    for _ in range(int(rng.integers(1, 5))):
        ops.append((pick(rng, [M, M, EQ, X]), pick(rng, MATCH_LEN)))
        k = int(rng.integers(0, 12))
        if k < 4:
            ops.append(([I, D, N, P][k], pick(rng, SKIP_LEN)))
        elif k == 4:
            ops.append((int(rng.integers(9, 16)), pick(rng, SKIP_LEN)))
        elif k == 5:
            ops.append((N, pick(rng, SKIP_LEN)))
            ops.append((pick(rng, [I, D]), pick(rng, SKIP_LEN)))
    return ops


def _indel_head(rng):
    """`S? (I|D)` or `M N (I|D)`: the forms whose indel claims (one behind the read's own match is refused)"""
    indel = (pick(rng, [I, D]), pick(rng, SKIP_LEN))
    if rng.random() < 0.5:
        return ([(S, pick(rng, SKIP_LEN))] if rng.random() < 0.5 else []) + [indel], 0
    a = pick(rng, [x for x in MATCH_LEN if x <= 129])
    b = pick(rng, [x for x in SKIP_LEN if x <= 129 and (x or not a)])  # a skip of 0 behind a match: the match holds the anchor
    return [(pick(rng, [M, EQ, X]), a), (N, b), indel], a + b


def _flags(rng):
    return (16 if rng.random() < 0.5 else 0) | (1024 if rng.random() < 0.05 else 0) | (512 if rng.random() < 0.05 else 0) | (4 if rng.random() < 0.03 else 0)


def _sample_reads(rng, window, ge, lead):
    """8-16 reads, sorted by position as a BAM file holds them.  `lead`: before them stands an indel form whose anchor lies inside
    the window and which passes every filter, so that it claims and the round's tokens do not hang on chance (records are taken
    in file order, whatever their positions: the definition asks for no sorting)."""
    beg, end = window
    n_reads = int(rng.integers(8, 17))
    lo = beg - 250
    reads = []
    if lead:
        anchor = int(rng.integers(beg, min(end, ge - 1) + 1))  # (an indel anchored on the step's last base is lost)
        while True:
            head, span = _indel_head(rng)
            if anchor - span >= lo:
                break
        cigar = ([(H, 2)] if rng.random() < 0.1 else []) + head + _body(rng)
        reads.append(make_read(rng, anchor - span, cigar, mapq=pick(rng, [pr.MAPQ_THD, 37, 60, 255]), flag=16 if rng.random() < 0.5 else 0))
    while len(reads) < n_reads:
        k = len(reads)
        head = _indel_head(rng)[0] if k % 3 == 0 else ([(S, pick(rng, SKIP_LEN))] if rng.random() < 0.3 else [])
        cigar = ([(H, 2)] if rng.random() < 0.1 else []) + head + _body(rng) + ([(S, 2)] if rng.random() < 0.2 else [])
        reads.append(make_read(rng, int(rng.integers(lo, end + 51)), cigar, mapq=pick(rng, [pr.MAPQ_THD - 1, pr.MAPQ_THD, 37, 60, 255]), flag=_flags(rng)))
    reads = reads[:1] + sorted(reads[1:], key=lambda r: r["pos"]) if lead else sorted(reads, key=lambda r: r["pos"])
    # other contigs before and behind, as in the corpus of pileup_ref: skipped, and the end of the sample
    if rng.random() < 0.3:
        reads.insert(0, make_read(rng, int(rng.integers(0, 1900)), [(M, 50)], tid=0))
    if rng.random() < 0.3:
        reads.append(make_read(rng, 10, [(M, 30)], tid=2))
    return reads


def campaign_window(rng, seed):
    rows = WINDOW_ROWS[seed % len(WINDOW_ROWS)] if rng.random() < 0.7 else pick(rng, WINDOW_ROWS)
    kind = int(rng.integers(0, 6))
    if kind == 0:    # abuts the first row of the second step: reads begin before the step, i_lo > 0
        beg = GB2
    elif kind == 1:  # abuts the last row of the first step (not with one row: an indel anchored there is lost)
        rows = max(rows, 31)
        beg = GB2 - rows
    else:
        base = pick(rng, [1000, 1200, 1400, 1600, 498000, 520000])
        beg = base - base % 32 + int(rng.integers(0, 32)) + 32
    return beg, beg + rows - 1


def campaign_round(seed):
    """One valid round, seeded from `seed` alone: (runs, run_sample, n_samples, window, ref)"""
    rng = np.random.default_rng([seed, 77])
    n = N_SAMPLES[(seed // 7) % len(N_SAMPLES)] if rng.random() < 0.7 else pick(rng, N_SAMPLES)
    window = campaign_window(rng, seed)
    ge = pr.step_of(window)[1]
    # samples without a run: about one in seven from five samples on, sample 0 / the last one in a third of the rounds each
    without = set()
    if n >= 5:
        forced = {0: 0, 1: n - 1}.get(seed % 3)
        if forced is not None:
            without.add(forced)
        while len(without) < max(1, round(n / 7)):
            without.add(int(rng.integers(0, n)))
    with_runs = [s for s in range(n) if s not in without]
    leads = set(rng.permutation(with_runs)[:(len(with_runs) + 1) // 2].tolist())
    runs, run_sample = [], []
    for s in with_runs:
        recs = [pack(r) for r in _sample_reads(rng, window, ge, s in leads)]
        cuts = sorted(int(x) for x in rng.integers(0, len(recs) + 1, int(rng.integers(0, 3))))  # 1-3 runs, empty ones too
        for a, b in zip([0] + cuts, cuts + [len(recs)]):
            runs.append(b"".join(recs[a:b]))
            run_sample.append(s)
    # the reference: in a third of the rounds it ends a little behind the window, inside its step: deleted bases are clipped
    ref_len = window[1] + pick(rng, [0, 1, 50, 300]) if rng.random() < 0.34 else window[1] + 3000
    return runs, run_sample, n, window, FA[:min(ref_len, len(FA))].encode()


def pack_is_record_bytes(seed=CAMPAIGN_SEEDS[0]):
    """pack against pr.record_bytes on one sample's reads of a round"""
    rng = np.random.default_rng([seed, 78])
    reads = _sample_reads(rng, (1040, 1103), 500000, True)
    return all(pack(r) == pr.record_bytes(dict(r, qual=[int(q) for q in r["qual"]])) for r in reads)


# ----------------------------------------------------------------------------------------------------------------- directed cases
class Case:
    """One hand-built case.  recs: per sample the reads as dicts where the case is a valid BAM file a sample (else None);
    expect: what the case itself states of its answer -- status (and sample, run, at) of a damaged one, `tokens` {(pos, sample):
    text}, `cells` {(pos, sample): (cell, qual or None, rank or None)}, `uncovered` [sample, ...]"""

    def __init__(self, runs, run_sample, n_samples, window, ref, recs=None, **expect):
        self.runs, self.run_sample, self.n_samples, self.window, self.ref = runs, run_sample, n_samples, window, ref
        self.recs, self.expect = recs, expect

    def tuple(self):
        return self.runs, self.run_sample, self.n_samples, self.window, self.ref

    @property
    def status(self):
        return self.expect.get("status", 0)


def small_run(rng):
    return [pr.read(rng, 1000 + 3 * k, [(S, 1), (I, 1), (M, 3)]) for k in range(3)]


def patched(b, at, fmt, v):
    return b[:at] + np.array([v], fmt).tobytes() + b[at + np.dtype(fmt).itemsize:]


def _of_samples(samples, window, ref=None, bam=True, **expect):
    """a case of one run a sample (a sample without reads has none)"""
    runs = [b"".join(pr.record_bytes(r) for r in recs) for recs in samples if recs]
    return Case(runs, [s for s, recs in enumerate(samples) if recs], len(samples), window, (ref if ref is not None else FA[:4000]).encode(),
                recs=samples if bam else None, **expect)


@functools.lru_cache(maxsize=None)
def directed():
    rng = np.random.default_rng(4242)
    W = (1000, 1999)
    c = {}
    rd = lambda *a, **kw: pr.read(rng, *a, **kw)
    tok = lambda sign, anchor, text: sign + FA[anchor - 1] + text

    # -- text and strides
    dels = [rd(1240, [(D, 65), (M, 10)]), rd(1400, [(D, 300), (M, 10)], flag=16), rd(1480, [(S, 2), (D, 129), (M, 4)])]
    c["long_deletions"] = _of_samples([dels], W, tokens={(1240, 0): tok("-", 1240, FA[1240:1305]), (1400, 0): tok("-", 1400, FA[1400:1700]),
                                                         (1480, 0): tok("-", 1480, FA[1480:1609])},
                                      cells={(1240, 0): (0x0A, None, 1), (1400, 0): (0x0E, None, 1), (1480, 0): (0x0A, None, 3)})
    assert FA[1270].islower() and FA[1550].islower() and "N" in FA[1400:1700]
    c["deletion_clipped_by_the_reference"] = _of_samples([[rd(1050, [(D, 200), (M, 5)])]], (1000, 1063), ref=FA[:1120], bam=False,
                                                         tokens={(1050, 0): tok("-", 1050, FA[1050:1120])})
    ins = [rd(1010 + 40 * k, [(S, 3), (I, ln), (M, 10)]) for k, ln in enumerate((64, 65, 129, 300))]
    c["long_insertions"] = _of_samples([ins], W, tokens={(1010 + 40 * k, 0): tok("+", 1010 + 40 * k, r["seq"][3:3 + r["cigar"][1][1]]) for k, r in enumerate(ins)},
                                       cells={(1010 + 40 * k, 0): (0x09, None, 4) for k in range(4)})
    short = rd(1020, [(S, 8), (I, 300), (D, 1)], seq="ACGTN" * 20, qual=[30] * 100)
    c["insertion_clipped_by_l_seq"] = _of_samples([[short]], W, bam=False, tokens={(1020, 0): tok("+", 1020, ("ACGTN" * 20)[8:])})
    odd = rd(1030, [(S, 1), (I, 70), (M, 8)], seq="A" + "=MRSVWYHKDB" * 6 + "ACGT" + "ACGTNACG")
    c["insertion_of_other_nibbles"] = _of_samples([[odd]], W, tokens={(1030, 0): tok("+", 1030, " " * 66 + "ACGT")})

    # -- quality
    q = [[rd(1100, [(I, 2), (M, 30)], qual=[255] * 32)], [rd(1100, [(S, 1), (D, 4), (M, 30)], qual=[0] * 31)]]
    c["quals_255_and_0"] = _of_samples(q, W, cells={(1100, 0): (0x09, 255, 1), (1101, 0): (None, 255, 3), (1100, 1): (0x0A, 0, 2), (1105, 1): (None, 0, 2)})
    ls = [rd(1000 + 200 * k, [(I, 1)] + ([(M, ln - 1)] if ln > 1 else [])) for k, ln in enumerate((1, 3, 64, 65))]
    for r in ls:
        r["qual"] = [int(x) for x in np.random.default_rng(len(r["seq"])).integers(0, 256, len(r["seq"]))]
    c["l_seq_1_3_64_65"] = _of_samples([ls], W, cells={(1000 + 200 * k, 0): (0x09, sum(r["qual"]) // len(r["qual"]), 1) for k, r in enumerate(ls)})
    ms = [rd(1000, [(I, 1), (M, 2)], qual=[10, 10, 10]), rd(1100, [(I, 1), (M, 2)], qual=[10, 10, 9]),
          rd(1200, [(I, 1), (M, 64)], qual=[198] * 32 + [200] * 32 + [199]), rd(1400, [(I, 1), (M, 64)], qual=[198] * 32 + [200] * 32 + [198])]
    assert sum(ms[2]["qual"]) == 199 * 65 and sum(ms[3]["qual"]) == 199 * 65 - 1
    c["mean_quality_at_a_whole_number"] = _of_samples([ms], W, cells={(1000, 0): (0x09, 10, 1), (1100, 0): (0x09, 9, 1), (1200, 0): (0x09, 199, 1), (1400, 0): (0x09, 198, 1)})

    # -- odd records
    z = [rd(1000, [(S, 2), (I, 0), (M, 5)]), rd(1020, [(M, 0), (I, 0), (M, 3)]), rd(1040, [(D, 0), (M, 4)], flag=16)]
    c["zero_length_operations"] = _of_samples([z], W, tokens={(1000, 0): tok("+", 1000, ""), (1020, 0): tok("+", 1020, ""), (1040, 0): tok("-", 1040, "")},
                                              cells={(1000, 0): (0x09, None, 3), (1020, 0): (0x09, None, 1), (1040, 0): (0x0E, None, 1)})
    c["no_cigar"] = _of_samples([[rd(1010, [], seq="ACGTACGTAC", qual=[30] * 10), rd(1020, [(M, 10)])]], W, cells={(1010, 0): (8, 0, 0), (1011, 0): (8, 0, 0), (1021, 0): (None, None, 1)})
    start = [rd(-1, [(M, 10)], flag=4), rd(0, [(I, 2), (M, 10)]), rd(4, [(S, 1), (D, 2), (M, 10)]), rd(20, [(S, 1), (D, 2), (M, 10)])]
    c["contig_start"] = _of_samples([start], (1, 64), tokens={(20, 0): tok("-", 20, FA[20:22])},  # (the deletion anchored on base 4 finds it held)
                                    cells={(1, 0): (None, None, 3), (4, 0): (None, None, 6), (11, 0): (None, None, 6), (20, 0): (0x0A, None, 2), (23, 0): (None, None, 2)})
    c["operation_codes_9_and_15"] = _of_samples([[rd(1000, [(M, 5), (9, 3), (M, 5), (15, 2), (M, 5)])]], W,
                                                cells={(1001, 0): (None, None, 1), (1006, 0): (None, None, 6), (1015, 0): (None, None, 15), (1016, 0): (8, 0, 0)})
    c["mapq_255_and_0"] = _of_samples([[rd(1000, [(M, 20)], mapq=255)], [rd(1000, [(M, 20)], mapq=0)]], W, uncovered=[1], cells={(1001, 0): (None, None, 1)})

    # -- runs
    far, near = pr.record_bytes(rd(5000, [(M, 5)])), pr.record_bytes(rd(1010, [(I, 2), (M, 50)]))
    other = pr.record_bytes(rd(1010, [(M, 50)]))
    r0 = pr.record_bytes(small_run(rng)[0])
    bad_block = patched(r0, 0, "<u4", 5)
    fa = FA[:6000].encode()
    c["break_then_a_claimable_run"] = Case([far, near, other], [0, 0, 1], 2, W, fa, uncovered=[0])
    c["damaged_behind_a_break"] = Case([far, bad_block, other], [0, 0, 1], 2, W, fa, uncovered=[0])
    c["damaged_in_a_sample_of_its_own"] = Case([far, bad_block], [0, 1], 2, W, fa, status=pr.BAD_BLOCK, fail=(1, 1, 0))
    c["two_failing_samples"] = Case([other, near, b"", near + patched(r0, 4 + 16, "<i4", 1 << 20), bad_block], [0, 1, 1, 1, 2], 3, W, fa,
                                    status=pr.BAD_LENGTHS, fail=(1, 3, len(near)))

    # -- damaged records: every status
    c["bad_block"] = Case([near + patched(r0, 0, "<u4", 31)], [0], 1, W, fa, status=pr.BAD_BLOCK, fail=(0, 0, len(near)))
    c["bad_run"] = Case([near + r0[:-1]], [0], 1, W, fa, status=pr.BAD_RUN, fail=(0, 0, len(near)))
    c["bad_lengths"] = Case([patched(r0, 4 + 12, "<u2", 60000)], [0], 1, W, fa, status=pr.BAD_LENGTHS, fail=(0, 0, 0))
    c["bad_query_through_a_match"] = Case([pr.record_bytes(rd(1000, [(M, 50)], seq="ACGTACGTAC", qual=[30] * 10))], [0], 1, W, fa, status=pr.BAD_QUERY, fail=(0, 0, 0))
    c["bad_query_through_an_insertion"] = Case([pr.record_bytes(rd(1000, [(S, 20), (I, 2), (D, 1)], seq="ACGTACGTAC", qual=[30] * 10))], [0], 1, W, fa,
                                               status=pr.BAD_QUERY, fail=(0, 0, 0))
    # (the engine refuses a window that ends beyond the reference before any launch: this status is the core's alone)
    c["bad_ref"] = Case([pr.record_bytes(rd(1040, [(M, 10), (N, 1), (D, 5), (M, 5)]))], [0], 1, (1000, 1063), FA[:1045].encode(), status=pr.BAD_REF, fail=(0, 0, 0))
    c["bad_base"] = Case([near + pr.record_bytes(rd(1990, [(M, 40)], seq="ACGT" * 7 + "ACM" + "ACGTACGTA"))], [0], 1, W, fa, status=pr.BAD_BASE, fail=(0, 0, len(near)))
    return c


def tokens_of(d):
    return {(int(t["pos"]), int(t["sample"])): d.text[int(t["text_off"]):int(t["text_off"]) + int(t["text_len"])].tobytes().decode() for t in d.tokens}


def check_expectation(c, d):
    """what a hand-built case states of its own answer (d: the harness's Dump, or the device's result with the same fields)"""
    e = c.expect
    if "tokens" in e:
        assert tokens_of(d) == e["tokens"]
    for (pos, s), (cell, qual, rank) in e.get("cells", {}).items():
        row = pos - c.window[0]
        assert cell is None or int(d.cell[row, s]) == cell, (pos, s)
        assert qual is None or int(d.qual[row, s]) == qual, (pos, s)
        assert rank is None or int(d.rank[row, s]) == rank, (pos, s)
        assert cell is not None or int(d.cell[row, s]) < 8 or int(d.cell[row, s]) & 3 == 0  # a base
    for s in e.get("uncovered", []):
        assert (d.cell[:, s] == 8).all() and not d.rank[:, s].any()


def directed_cases():
    """{name: (runs, run_sample, n_samples, window, ref)}"""
    return {k: v.tuple() for k, v in directed().items()}


def truncations():
    """a three-record run cut at every byte: [(cut, the run, status)]"""
    recs = [pr.record_bytes(r) for r in small_run(np.random.default_rng(10))]
    run = b"".join(recs)
    ends = set(np.cumsum([len(r) for r in recs]).tolist()) | {0}
    starts = [0] + np.cumsum([len(r) for r in recs]).tolist()
    return [(cut, run[:cut], 0 if cut in ends else pr.BAD_RUN, max(s for s in starts if s <= cut)) for cut in range(len(run))]


# -------------------------------------------------------------------------------------------------------------------- many samples
def wide_round(n, long_rank=8191, seed=5):
    """reads with indels in the samples at which a row loop of n cells takes another step, and in a seeded 1 % of the rest; every
    other sample has no run.  Window of 100 rows; the last sample's first read is one match of `long_rank` bases that ends on the
    window's last row: the window's largest rank, in the row's last cell."""
    rng = np.random.default_rng([seed, n])
    window = (10016, 10115)
    chosen = sorted({s for s in (0, 1, 63, 64, 511, 512, 4095, 4096, n - 1) if s < n} | set(np.flatnonzero(rng.random(n) < 0.01).tolist()))
    runs, run_sample = [], []
    for s in chosen:
        reads = [make_read(rng, int(rng.integers(9950, 10100)), [(S, 2), (pick(rng, [I, D]), pick(rng, [1, 5, 65])), (M, 40), (N, 3), (I, 2), (M, 30)],
                           flag=16 if rng.random() < 0.5 else 0) for _ in range(3)]
        reads.sort(key=lambda r: r["pos"])
        if s == n - 1:
            reads.insert(0, make_read(rng, window[1] - long_rank, [(M, long_rank)]))
        runs.append(b"".join(pack(r) for r in reads))
        run_sample.append(s)
    return runs, run_sample, n, window, FA[:12000].encode()


def variant_round(n, seed=6):
    """about 300 covered rows whose read bases are random against the reference: most rows are variant sites"""
    rng = np.random.default_rng([seed, n])
    window = (2001, 2300)
    runs, run_sample = [], []
    for s in range(n):
        if n > 200 and rng.random() < 0.7:
            continue
        reads = [make_read(rng, int(rng.integers(1900, 2300)), [(M, 100), (N, 2), (D, 2), (M, 50)], mapq=pick(rng, [20, 37, 60]),
                           flag=16 if rng.random() < 0.5 else 0, seq="".join("ACGT"[i] for i in rng.integers(0, 4, 150)),
                           qual=rng.integers(5, 42, 150).astype(np.uint8)) for _ in range(2)]
        runs.append(b"".join(pack(r) for r in sorted(reads, key=lambda r: r["pos"])))
        run_sample.append(s)
    return runs, run_sample, n, window, FA[:4000].encode()


def long_read(length=66000, pos=1000, seed=66):
    """one match of 66,000 bases: query index 65,535, whose rank does not fit 16 bits, lies at position pos + 65,536"""
    return pr.read(np.random.default_rng(seed), pos, [(M, length)])
