"""GPU tests of the parse job (include/basevar_amd_text_job.h), through the C ABI.  In every case the
expected side is bv_engine_text_parse + bv_engine_text_submit on the rows of all files joined position-major, on the same
engine; the job is begun, fed the files in groups and finished, and must leave the same row_state, records, group records, cell
and phred planes, the same layout bit of the submitted slab and, with the token mode on, the same descriptors and text byte
for byte -- whatever the partition into adds and their order."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import text_tokens_model as ttm  # noqa: E402
from text_tokens_model import NOCALL, call, ind, letters, mkrow  # noqa: E402

SENTINEL = 0xA5
MAX_SAMPLES = 700


# ------------------------------------------------------------------------------------------------------------------ the corpus
FILE_SAMPLES = {1: [65], 2: [1, 200], 3: [2, 63, 64], 5: [64, 1, 65, 200, 2]}  # 1, 2, 63, 64, 65 and 200 samples, mixed in a job


def kinds_of(F, P):
    """what decides every position: 'plain', 'sum' (Depth 0 in every file but the last), 'zero' (Depth 0 everywhere: skipped)"""
    if P == 1:
        return [{1: "plain", 2: "sum", 3: "zero", 5: "plain"}[F]]
    if P == 2:
        return ["sum" if F > 1 else "zero", "plain"]
    return ["sum" if p % 7 == 3 and F > 1 else "zero" if p % 7 == 5 else "plain" for p in range(P)]


def random_sample(rng, covered=None, big_rank=False):
    u = rng.random() if covered is None else (0.9 if covered else 0.1)
    if u < 0.5:
        return NOCALL
    if u < 0.6 and not big_rank:
        return ind(b"+-"[rng.integers(2):][:1] + letters(int(rng.integers(0, 7)), int(rng.integers(4))), b"+-"[rng.integers(2):][:1])
    return call(b"ACGT"[rng.integers(4):][:1], b"+-"[rng.integers(2):][:1], bytes([33 + int(rng.integers(0, 60))]), b"%d" % rng.integers(0, 256),
                b"%d" % (9000 if big_rank else rng.integers(0, 101)))


def gen_batch(F, P, seed, big_rank_at=None):
    """big_rank_at = (position, file): one call there has rank 9,000 -- above BV_RPR_TAG_MAX_RANK, in one file only"""
    rng = np.random.default_rng(seed)
    fs, kinds = FILE_SAMPLES[F], kinds_of(F, P)
    rows, state = [], []
    for p, kind in enumerate(kinds):
        files = []
        for f, n in enumerate(fs):
            if kind == "zero" or (kind == "sum" and f < F - 1):
                s = [NOCALL] * n
            else:
                s = [random_sample(rng) for _ in range(n)]
                s[0] = random_sample(rng, covered=True, big_rank=big_rank_at == (p, f))
            files.append(mkrow(b"chr%d" % (F + 1), 1000 + p, b"ACGTN"[p % 5:][:1], s))
        rows.append(files)
        state.append(ttm.SKIP if kind == "zero" else 0)
    name = "F%d_P%d%s" % (F, P, "_bigrank" if big_rank_at else "")
    b = ttm.Batch(name, rows, fs, state)
    b.kinds, b.big_rank = kinds, big_rank_at is not None
    return b


SHAPES = [gen_batch(F, P, 100 * F + P) for F in (1, 2, 3, 5) for P in (1, 2, 65)]
SHAPES += [gen_batch(3, 2, 77, big_rank_at=(1, 1)), gen_batch(5, 65, 78, big_rank_at=(9, 3))]


def defects_batch(f_bad):
    """3 files; every odd position carries one defect of the existing parser in file f_bad, every even one is well-formed"""
    fs = [2, 3, 2]
    A = call()

    def good(chrom, pos, ref=b"A"):
        return [mkrow(chrom, pos, ref, [A, ind(b"+A")]), mkrow(chrom, pos, ref, [NOCALL, call(b"C", b"-"), A]), mkrow(chrom, pos, ref, [ind(b"-GG", b"-"), A])]

    def sub(row, col, fn):
        f = row.split(b"\t")
        f[col] = fn(f[col])
        return b"\t".join(f)

    samples = [[A, ind(b"+A")], [NOCALL, call(b"C", b"-"), A], [ind(b"-GG", b"-"), A]][f_bad]
    with_first = lambda s: [s] + samples[1:]  # noqa: E731
    long_chrom = b"chr7" + b"L" * 600
    defects = [
        ("chrom", lambda r, pos: mkrow(b"chr8", pos, b"A", samples)),
        ("pos", lambda r, pos: mkrow(b"chr7", pos + 1, b"A", samples)),
        ("ref", lambda r, pos: mkrow(b"chr7", pos, b"C", samples)),
        ("long_head_one", lambda r, pos: mkrow(long_chrom, pos, b"A", samples)),
        ("ten_fields", lambda r, pos: r + b"\tX"),
        ("ragged", lambda r, pos: sub(r, 6, lambda c: c[:-2])),
        ("empty_token", lambda r, pos: sub(r, 4, lambda c: c.replace(b" ", b"  ", 1))),
        ("mapq", lambda r, pos: mkrow(b"chr7", pos, b"A", with_first(call(mapq=b"256")))),
        ("rank", lambda r, pos: mkrow(b"chr7", pos, b"A", with_first(call(rank=b"65536")))),
        ("dot_strand", lambda r, pos: mkrow(b"chr7", pos, b"A", with_first(call(b"G", b".")), depth=2)),
    ]
    rows, state, names = [], [], []
    for k, (name, fn) in enumerate(defects):
        rows.append(good(b"chr7", 50 + 2 * k))
        state.append(0)
        names.append(None)
        r = good(b"chr7", 51 + 2 * k)
        r[f_bad] = fn(r[f_bad], 51 + 2 * k)
        rows.append(r)
        state.append(ttm.HOST)
        names.append(name)
    rows.append(good(long_chrom, 99))  # a head longer than 512 bytes in every file
    state.append(ttm.HOST)
    names.append("long_head_all")
    rows.append(good(b"chr7", 100))
    state.append(0)
    names.append(None)
    b = ttm.Batch("defects_f%d" % f_bad, rows, fs, state)
    b.defect = names
    return b


def lanes_batch():
    """3 files x 65 positions: CHROM of 1 .. 65 bytes moves every column over every lane; the token of (p, f) is 1, 2, 64 or 65
    bytes long, so that its first byte and the separator behind it fall on every lane in every file, and tokens cross the
    64-byte steps"""
    lens = [1, 2, 64, 65]
    rows = []
    for k in range(1, 66):
        chrom = b"c" * k
        rows.append([mkrow(chrom, 100 + k, b"G", [call(), ind(b"+" + letters(lens[(k + 0) % 4] - 1, k))]),
                     mkrow(chrom, 100 + k, b"G", [ind(b"-" + letters(lens[(k + 1) % 4] - 1, k), b"-"), NOCALL, call(b"T", b"-")]),
                     mkrow(chrom, 100 + k, b"G", [NOCALL, ind(b"+" + letters(lens[(k + 2) % 4] - 1, k)), ind(b"-")])])
    return ttm.Batch("lanes3", rows, [2, 3, 3])


LANES = lanes_batch()
CORPUS = {b.name: b for b in ttm.corpus()}  # the batches of the token tests: 'lengths' (tokens of 9,000 bytes), 'states' (skipped and host positions)


def sub_packed(b, first, K):
    """(text, row_off) of files [first, first + K) of the batch: what an add brings"""
    flat = [b.rows[p][first + k] + b"\n" for p in range(b.P) for k in range(K)]
    off = np.zeros(len(flat) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in flat])
    return np.frombuffer(b"".join(flat), np.uint8), off


def partitions(F):
    out = {"all": [(0, F)], "singles": [(f, 1) for f in range(F)]}
    if F >= 2:
        out["pairs"] = [(f, min(2, F - f)) for f in range(0, F, 2)]
        out["one_rest"] = [(0, 1), (1, F - 1)]
    return out


def orders(adds):
    """forward (file 0 first), reversed (file 0 last), interleaved (file 0 in the middle where there are three adds or more)"""
    out = [adds, adds[::-1], adds[1::2] + adds[0::2]]
    return [o for k, o in enumerate(out) if o not in out[:k]]


# ------------------------------------------------------------------------------------------------------------------ the two sides
@pytest.fixture(scope="module")
def eng():
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=65, min_af_value=bv.min_af(MAX_SAMPLES), device=0, max_samples=MAX_SAMPLES)
    yield e
    e.close()


@contextlib.contextmanager
def token_mode(eng, on):
    if on:
        eng.text_tokens_enable(True)
    try:
        yield
    finally:
        if on:
            eng.text_tokens_enable(False)


def host_reader_for(file_samples):
    """A host reader that takes every defective row of this file's corpora: a file's columns are cut or filled to its sample
    count, numbers are clamped.  Both sides of every comparison are handed the same lines and use the same reader."""
    def reader(lines):
        if lines[0].startswith(b"skipme"):
            return None
        cell, phred, mapq, rank = [], [], [], []
        for ln, n in zip(lines, file_samples):
            cols = [[t for t in x.split(b" ") if t] for x in (ln.split(b"\t") + [b""] * 9)[4:9]]
            for i in range(n):
                m, bq, q, k, s = [c[i] if i < len(c) else d for c, d in zip(cols, NOCALL)]
                c = {b"A": 0, b"C": 1, b"G": 2, b"T": 3}.get(bq, 9 if bq[:1] == b"+" else 10 if bq[:1] == b"-" else 8)
                cell.append(c | 4 if c < 4 and s == b"-" else c)
                phred.append(q[0] - 33)
                mapq.append(min(int(m), 255))
                rank.append(min(int(k), 65535))
        ref = lines[0].split(b"\t")[2][:1].upper()
        return (np.array(cell, np.uint8), np.array(phred, np.uint8), np.array(mapq, np.uint8), np.array(rank, np.uint16), b"ACGT".find(ref) if ref in b"ACGT" and ref else 4)
    return reader


def gid_of(b, ng):
    return (np.arange(b.N) % ng).astype(np.uint8) if ng else None


def raw_fetch(eng):
    """bv_engine_text_tokens_fetch into exact buffers with sentinels around both: (descriptor bytes, text bytes)"""
    from basevar_amd import _capi
    item = _capi.PILEUP_TOKEN_DTYPE.itemsize
    n, nb = C.c_uint64(0), C.c_uint64(0)
    rc = eng._lib.bv_engine_text_tokens_fetch(eng._h, None, 0, None, 0, C.byref(n), C.byref(nb), None)
    assert rc == 0 or n.value
    n_cap, t_cap = int(n.value), int(nb.value)
    tok = np.full((n_cap + 2) * item, SENTINEL, np.uint8)
    text = np.full(t_cap + 64, SENTINEL, np.uint8)
    assert eng._lib.bv_engine_text_tokens_fetch(eng._h, tok.ctypes.data + item, n_cap, text.ctypes.data + 32, t_cap, C.byref(n), C.byref(nb), None) == 0
    assert (n.value, nb.value) == (n_cap, t_cap)
    assert (tok[:item] == SENTINEL).all() and (tok[(n_cap + 1) * item:] == SENTINEL).all()
    assert (text[:32] == SENTINEL).all() and (text[32 + t_cap:] == SENTINEL).all()
    return tok[item:(n_cap + 1) * item].tobytes(), text[32:32 + t_cap].tobytes()


def snapshot(eng, batch, tokens):
    """everything that is compared, as bytes"""
    layout = C.c_uint32(0xFFFF)
    if batch.sites.size:
        assert eng._lib.bv_engine_text_last_layout(eng._h, C.byref(layout)) == 0
    out = {"row_state": batch.row_state.tobytes(), "positions": batch.positions.tobytes(), "sites": batch.sites.tobytes(),
           "groups": b"" if batch.groups is None else batch.groups.tobytes(), "cell": batch.cell.tobytes(), "phred": batch.phred.tobytes(),
           "layout": layout.value, "n_variant": batch.n_variant}
    if tokens:
        out["tokens"], out["token_text"] = raw_fetch(eng)
    return out


def whole(eng, b, ng=0, tokens=False):
    """the expected side: bv_engine_text_parse + bv_engine_text_submit on the joined rows"""
    with token_mode(eng, tokens):
        got = eng.lrt_text(b.packed(), b.file_samples, group_id=gid_of(b, ng), n_groups=ng, host_reader=host_reader_for(b.file_samples))
        return snapshot(eng, got, tokens), got


def job(eng, b, adds, ng=0, tokens=False, between=None):
    """the job through its three calls, then bv_engine_text_submit; `between(k)` runs before add k"""
    from basevar_amd import _capi
    fs = np.asarray(b.file_samples, np.uint32)
    with token_mode(eng, tokens):
        eng.text_job_begin(b.P, fs, gid_of(b, ng), ng)
        flags = {}
        for k, (first, K) in enumerate(adds):
            if between:
                between(k)
            flags[first] = eng.text_job_add(sub_packed(b, first, K), fs[first:first + K], first)
        state = eng.text_job_finish(b.P, b.F)
        for first, fl in flags.items():  # row_flag: the marks of the add's rows, where the position was parsed
            for p in np.nonzero(state[:, 0] & (_capi.BV_TEXT_SKIP | _capi.BV_TEXT_HOST) == 0)[0]:
                assert fl[p].tolist() == (state[p, first:first + fl.shape[1]] & _capi.BV_TEXT_INDEL).tolist(), (b.name, first, p)
        got = eng._text_submit("job", state, b.P, b.F, b.N, ng, host_reader_for(b.file_samples), lambda p: list(b.rows[p]))
        return snapshot(eng, got, tokens), got


def same(got, exp, what):
    for k in exp:
        assert got[k] == exp[k], (what, k)


def states_are_the_corpus(b, batch):
    from basevar_amd import _capi
    final = batch.row_state[:, 0] & (_capi.BV_TEXT_SKIP | _capi.BV_TEXT_HOST)
    assert final.tolist() == b.state, b.name


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("ng", [0, 2])
@pytest.mark.parametrize("tokens", [False, True], ids=["tokens_off", "tokens_on"])
@pytest.mark.parametrize("b", SHAPES, ids=[b.name for b in SHAPES])
def test_every_partition_and_order_gives_the_whole_parse(eng, b, tokens, ng):
    from basevar_amd import _capi
    exp, batch = whole(eng, b, ng, tokens)
    states_are_the_corpus(b, batch)
    if batch.sites.size:  # a rank above 8,191 in one file only: the submit comes out plain, not tagged
        assert exp["layout"] == (0 if b.big_rank else _capi.BV_SLAB_RPR_TAGGED)
    if "sum" in b.kinds:  # decided by the sum alone: Depth 0 in every file of one add, positive in another -- and called
        p = b.kinds.index("sum")
        assert all(int(r.split(b"\t")[3]) == 0 for r in b.rows[p][:-1]) and int(b.rows[p][-1].split(b"\t")[3]) > 0 and p in batch.positions
    if tokens:
        assert ttm.tokens_of_arrays(np.frombuffer(exp["tokens"], _capi.PILEUP_TOKEN_DTYPE), np.frombuffer(exp["token_text"], np.uint8)) == b.tokens()
    for pname, adds in partitions(b.F).items():
        for order in orders(adds):
            same(job(eng, b, order, ng, tokens)[0], exp, (b.name, pname, order))


@pytest.mark.parametrize("f_bad", [0, 1, 2])
def test_defects_in_the_first_a_middle_and_the_last_added_file(eng, f_bad):
    """every defect of the existing parser, in file f_bad: added first, in the middle and last (file 0 in each of the three)"""
    from basevar_amd import _capi
    b = defects_batch(f_bad)
    for tokens in (False, True):
        exp, batch = whole(eng, b, 0, tokens)
        for p, name in enumerate(b.defect):  # a corpus that misses its case fails here
            assert (batch.row_state[p] & _capi.BV_TEXT_HOST).all() == (name is not None), (p, name)
        states_are_the_corpus(b, batch)
        for order in ([(0, 1), (1, 1), (2, 1)], [(2, 1), (1, 1), (0, 1)], [(1, 1), (0, 1), (2, 1)], [(1, 1), (2, 1), (0, 1)], [(0, 2), (2, 1)], [(1, 2), (0, 1)]):
            same(job(eng, b, order, 0, tokens)[0], exp, (b.name, order))


def lane_cases(b, f):
    """(lanes of the tokens' first bytes, lanes of their ending separators, a token crosses a 64-byte step, token lengths) in file f"""
    first, end, crosses, lens = set(), set(), False, set()
    for p in range(b.P):
        for a, e in ttm.token_places(b.rows[p][f]):
            first.add(a % 64)
            end.add(e % 64)
            crosses |= a // 64 != (e - 1) // 64
            lens.add(e - a)
    return first, end, crosses, lens


@pytest.mark.parametrize("name", ["lanes3", "lengths", "states"])
def test_tokens_in_every_place_of_an_add(eng, name):
    """the list, in both modes: every file is the first of an add, the last of one, and lies in adds on either side of another"""
    from basevar_amd import _capi
    b = LANES if name == "lanes3" else CORPUS[name]
    assert b.F == 3
    if name == "lanes3":
        for f in range(3):
            first, end, crosses, lens = lane_cases(b, f)
            assert {0, 1, 62, 63} <= first and {0, 1, 62, 63} <= end and crosses and {1, 2, 64, 65} <= lens, f
    if name == "lengths":
        assert 9000 in lane_cases(b, 1)[3]
    exp, batch = whole(eng, b, 0, True)
    states_are_the_corpus(b, batch)
    want = b.tokens()
    assert ttm.tokens_of_arrays(np.frombuffer(exp["tokens"], _capi.PILEUP_TOKEN_DTYPE), np.frombuffer(exp["token_text"], np.uint8)) == want
    if name == "states":  # tokens of a position that ends skipped or host-read are absent
        gone = {p for p in range(b.P) if b.state[p]}
        assert gone and any(ttm.marked(r) for p in gone for r in b.rows[p]) and not gone & {p for p, s, t in want}
    with token_mode(eng, True):  # (turning the mode off kept the whole parse's list)
        tok, text = eng.text_tokens()
        exp_off, exp_flag = eng.indel_tally(batch.positions, tok, text)
        exp_cols = eng.indel_fetch().tobytes()
    exp_plain = whole(eng, b, 0, False)[0]
    for pname, adds in partitions(3).items():
        for order in orders(adds):
            same(job(eng, b, order, 0, True)[0], exp, (name, pname, order))
            with token_mode(eng, True):  # indel_tally over the job's list is the tally over the whole parse's
                tok, text = eng.text_tokens()
                off, flag = eng.indel_tally(batch.positions, tok, text)
                assert np.array_equal(off, exp_off) and np.array_equal(flag, exp_flag) and eng.indel_fetch().tobytes() == exp_cols
            same(job(eng, b, order, 0, False)[0], exp_plain, (name, pname, order, "mode off"))


def test_adds_cut_into_chunks():
    """BASEVAR_AMD_TEXT_CHUNK_BYTES cuts every add of 65 positions into three chunks and more, on an engine of its own (the stage
    only grows: on the shared engine it would cut nothing)"""
    import basevar_amd as bv
    b = LANES
    chunk = 2048
    for first, K in ((0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (0, 3)):
        part = ttm.Batch("part", [r[first:first + K] for r in b.rows], b.file_samples[first:first + K], chunk_bytes=chunk)
        assert len(part.chunks(cap_before=chunk)) >= 3 and len(part.chunks()) >= 3, (first, K)
    old = os.environ.get("BASEVAR_AMD_TEXT_CHUNK_BYTES")
    os.environ["BASEVAR_AMD_TEXT_CHUNK_BYTES"] = str(chunk)
    e = bv.BaseTypeEngine(max_sites=65, min_af_value=bv.min_af(64), device=0, max_samples=64)
    try:
        for tokens in (True, False):
            for ng in (0, 2):
                got = job(e, b, [(2, 1), (0, 2)], ng, tokens)[0]  # (first: the stage is no larger than a chunk)
                exp = whole(e, b, ng, tokens)[0]
                same(got, exp, ("chunks", tokens, ng))
                for pname, adds in partitions(3).items():
                    for order in orders(adds):
                        same(job(e, b, order, ng, tokens)[0], exp, ("chunks", pname, order, tokens, ng))
    finally:
        e.close()
        if old is None:
            del os.environ["BASEVAR_AMD_TEXT_CHUNK_BYTES"]
        else:
            os.environ["BASEVAR_AMD_TEXT_CHUNK_BYTES"] = old


def test_refusals_leave_the_job_as_it_was(eng):
    from basevar_amd import _capi
    INVALID = _capi.BV_ERR_INVALID_ARG
    lib, h = eng._lib, eng._h
    b = CORPUS["states"]
    fs = np.asarray(b.file_samples, np.uint32)
    exp = whole(eng, b, 2, True)[0]
    state = np.zeros((b.P, b.F), np.uint8)

    def rows_of(first, K, **kw):
        text, off = sub_packed(b, first, K)
        keep = [text, off, np.ascontiguousarray(kw.pop("file_samples", fs[first:first + K]), np.uint32)]
        tr = _capi.TextRows(text.ctypes.data, off.ctypes.data, keep[2].ctypes.data, int(text.size), b.P, K, 0)
        for k, v in kw.items():
            setattr(tr, k, v)
        return tr, keep

    def refused(rc, *words):
        assert rc == INVALID
        msg = eng._err()
        assert all(w in msg for w in words), msg

    # ---- no job: after a whole parse, add and finish are refused, and the parse's submit state is untouched
    tr, keep = rows_of(0, 1)
    refused(lib.bv_engine_text_job_add(h, C.byref(tr), 0, None, None), "bv_engine_text_job_add", "no open job")
    refused(lib.bv_engine_text_job_finish(h, state.ctypes.data, None), "bv_engine_text_job_finish", "no open job")
    # ---- begin's own
    gid = gid_of(b, 2)
    refused(lib.bv_engine_text_job_begin(h, b.P, b.F, None, None, 0, None), "null file_samples")
    refused(lib.bv_engine_text_job_begin(h, 0, b.F, fs.ctypes.data, None, 0, None), "must be > 0")
    refused(lib.bv_engine_text_job_begin(h, 66, b.F, fs.ctypes.data, None, 0, None), "cfg.max_sites")
    big = np.asarray([MAX_SAMPLES, 1], np.uint32)
    refused(lib.bv_engine_text_job_begin(h, b.P, 2, big.ctypes.data, None, 0, None), "cfg.max_samples")
    refused(lib.bv_engine_text_job_begin(h, b.P, b.F, fs.ctypes.data, gid.ctypes.data, 0, None), "group_id")
    refused(lib.bv_engine_text_job_begin(h, b.P, b.F, fs.ctypes.data, None, 2, None), "group_id")

    def during(k):
        """between the adds of an open job (files 1, then 0, then 2): every refusal, each leaving the job to go on"""
        if k == 0:
            return
        refused(lib.bv_engine_text_job_finish(h, state.ctypes.data, None), "missing")   # files are missing: the job stays open
        refused(lib.bv_engine_text_job_finish(h, None, None), "null row_state")
        tr, keep = rows_of(1, 1)
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 1, None, None), "file 1 was added before")
        tr, keep = rows_of(1, 2)
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 1, None, None), "added before")  # a range that touches it
        tr, keep = rows_of(2, 1)
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 3, None, None), "beyond")
        tr, keep = rows_of(0, 3)
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 1, None, None), "beyond")
        tr, keep = rows_of(2, 1, n_positions=b.P - 1)
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 2, None, None), "n_positions")
        tr, keep = rows_of(2, 1, file_samples=[fs[2] + 1])
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 2, None, None), "file_samples")
        tr, keep = rows_of(2, 1, reserved_=1)
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 2, None, None), "reserved_")
        tr, keep = rows_of(2, 1, text=None)
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 2, None, None), "null text")
        refused(lib.bv_engine_text_job_add(h, None, 2, None, None), "null rows")
        tr, keep = rows_of(2, 1)
        tr.text_bytes -= 1
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 2, None, None), "row_off outside text_bytes")
        tr, keep = rows_of(2, 1)
        keep[1][3] = keep[1][2]  # offsets out of order
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 2, None, None), "out of order")
        tr, keep = rows_of(2, 1)
        text = keep[0].copy()
        text[int(keep[1][1]) - 1] = ord("x")  # no final line break
        tr.text = text.ctypes.data
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 2, None, None), "no final")
        eng.text_tokens_enable(False)  # the token mode changed since begin
        tr, keep = rows_of(2, 1)
        refused(lib.bv_engine_text_job_add(h, C.byref(tr), 2, None, None), "token mode")
        eng.text_tokens_enable(True)

    same(job(eng, b, [(1, 1), (0, 1), (2, 1)], 2, True, between=during)[0], exp, "refusals between the adds")
    # ---- a finish refused for missing files, then the missing add, then finish
    with token_mode(eng, True):
        eng.text_job_begin(b.P, fs, gid, 2)
        eng.text_job_add(sub_packed(b, 0, 2), fs[:2], 0)
        refused(lib.bv_engine_text_job_finish(h, state.ctypes.data, None), "1 of the job's 3 files are missing", "file 2")
        eng.text_job_add(sub_packed(b, 2, 1), fs[2:], 2)
        st = eng.text_job_finish(b.P, b.F)
        got = eng._text_submit("job", st, b.P, b.F, b.N, 2, ttm.host_reader, lambda p: list(b.rows[p]))
        same(snapshot(eng, got, True), exp, "finish after the missing add")
        refused(lib.bv_engine_text_job_finish(h, state.ctypes.data, None), "no open job")  # one finish per job
    # ---- an abandoned job: a new begin, and a plain parse, replace it
    eng.text_job_begin(b.P, fs, None, 0)
    eng.text_job_add(sub_packed(b, 1, 1), fs[1:2], 1)
    same(job(eng, b, [(0, 3)], 2, True)[0], exp, "a begin abandons the open job")
    eng.text_job_begin(b.P, fs, None, 0)
    eng.text_job_add(sub_packed(b, 1, 1), fs[1:2], 1)
    same(whole(eng, b, 2, True)[0], exp, "a parse abandons the open job")
    tr, keep = rows_of(0, 1)
    refused(lib.bv_engine_text_job_add(h, C.byref(tr), 0, None, None), "no open job")
    assert lib.bv_engine_text_job_begin(None, 1, 1, fs.ctypes.data, None, 0, None) == INVALID
    assert lib.bv_engine_text_job_add(None, C.byref(tr), 0, None, None) == INVALID
    assert lib.bv_engine_text_job_finish(None, state.ctypes.data, None) == INVALID


def test_lrt_text_job_is_lrt_text(eng):
    """the wrapper: a host-read position between device-parsed ones, in both token modes; and a host reader that throws at a
    position with device-parsed positions before and behind it -- the same error, and the engine goes on"""
    b = CORPUS["states"]
    assert b.state[2:5] == [0, ttm.HOST, 0]
    for tokens in ("host", "device"):
        exp = eng.lrt_text(b.packed(), b.file_samples, host_reader=ttm.host_reader, tokens=tokens)
        for adds in ([(2, [r[2:] for r in b.rows]), (0, [r[:2] for r in b.rows])], [(1, sub_packed(b, 1, 2), 2), (0, sub_packed(b, 0, 1), 1)]):
            got = eng.lrt_text_job(adds, b.file_samples, host_reader=ttm.host_reader, tokens=tokens)
            assert np.array_equal(got.row_state, exp.row_state) and np.array_equal(got.positions, exp.positions)
            assert got.sites.tobytes() == exp.sites.tobytes() and got.n_variant == exp.n_variant
            assert got.cell.tobytes() == exp.cell.tobytes() and got.phred.tobytes() == exp.phred.tobytes()
            if tokens == "device":
                assert got.tokens.tobytes() == exp.tokens.tobytes() and got.token_text.tobytes() == exp.token_text.tobytes()

    seen = []

    def throwing(lines):
        seen.append(lines)
        if lines[0].split(b"\t")[1] == b"895":  # position 5
            raise ValueError("the host reader refuses position 895")
        return ttm.host_reader(lines)

    with pytest.raises(ValueError, match="895"):
        eng.lrt_text(b.packed(), b.file_samples, host_reader=throwing)
    seen_whole, seen[:] = list(seen), []
    with pytest.raises(ValueError, match="895"):
        eng.lrt_text_job([(2, [r[2:] for r in b.rows]), (0, [r[:2] for r in b.rows])], b.file_samples, host_reader=throwing)
    assert seen == seen_whole and len(seen) == 2  # the same positions' lines, all files in file order, up to the throw
    got = eng.lrt_text_job([(0, [list(r) for r in b.rows])], b.file_samples, host_reader=ttm.host_reader)
    assert got.sites.tobytes() == eng.lrt_text(b.packed(), b.file_samples, host_reader=ttm.host_reader).sites.tobytes()
