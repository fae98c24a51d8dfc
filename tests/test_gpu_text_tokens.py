"""GPU tests of the text tokens taken on the device (include/basevar_amd_text_tokens.h), all through the C ABI: over the corpus of
tests/text_tokens_model.py the fetched list and the list behind the device pointers are the serial model's; the BGZF route gives
the text route's list; records, row states and planes are the default calls'; the heads fetch is the rows fetch with marked rows
cut; the tally over the device tokens is indel_string of the host walk's tokens; and every refusal leaves the last list usable."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bgzf_corpus as bc  # noqa: E402
import indel_tally_ref as itr  # noqa: E402
import text_tokens_model as ttm  # noqa: E402

SENTINEL = 0xA5
CORPUS = ttm.corpus()  # built once, left unchanged
NAMES = [b.name for b in CORPUS]


@pytest.fixture(scope="module")
def eng():
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=65, min_af_value=bv.min_af(512), device=0, max_samples=512)
    yield e
    e.close()


def batch(name):
    return CORPUS[NAMES.index(name)]


@contextlib.contextmanager
def engine_for(eng, b):
    """The shared engine -- or, for a batch that is there for its chunks, an engine of its own: the chunk stage only grows, so on
    an engine that has parsed a larger batch BASEVAR_AMD_TEXT_CHUNK_BYTES cuts nothing and the batch would go through whole"""
    if not b.chunk_bytes:
        yield eng
        return
    import basevar_amd as bv
    assert len(b.chunks()) >= 3 and len(b.chunks(cap_before=1 << 14)) == 1
    fresh = bv.BaseTypeEngine(max_sites=65, min_af_value=bv.min_af(512), device=0, max_samples=512)
    try:
        yield fresh
    finally:
        fresh.close()


def lrt_text(eng, b, **kw):
    old = os.environ.get("BASEVAR_AMD_TEXT_CHUNK_BYTES")
    if b.chunk_bytes:
        os.environ["BASEVAR_AMD_TEXT_CHUNK_BYTES"] = str(b.chunk_bytes)
    try:
        return eng.lrt_text(b.packed(), b.file_samples, host_reader=ttm.host_reader, **kw)
    finally:
        if b.chunk_bytes:
            if old is None:
                del os.environ["BASEVAR_AMD_TEXT_CHUNK_BYTES"]
            else:
                os.environ["BASEVAR_AMD_TEXT_CHUNK_BYTES"] = old


def same_batch(got, exp):
    assert np.array_equal(got.row_state, exp.row_state) and np.array_equal(got.positions, exp.positions)
    assert got.sites.tobytes() == exp.sites.tobytes() and got.n_variant == exp.n_variant
    assert got.cell.tobytes() == exp.cell.tobytes() and got.phred.tobytes() == exp.phred.tobytes()


def states_are_the_corpus(b, got):
    """the parse's row states are what the batch was built for: the model's input is not the device's word"""
    from basevar_amd import _capi
    final = got.row_state[:, 0] & (_capi.BV_TEXT_SKIP | _capi.BV_TEXT_HOST)
    assert final.tolist() == b.state, b.name
    for p in range(b.P):
        if not b.state[p]:
            assert [bool(s & _capi.BV_TEXT_INDEL) for s in got.row_state[p]] == [ttm.marked(r) for r in b.rows[p]], (b.name, p)
    assert got.positions.tolist() == [p for p in range(b.P) if b.state[p] != ttm.SKIP]


def hip_runtime():
    """the HIP runtime this process has loaded (torch's), for reading device memory back"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def device_read(ptr, n):
    out = np.zeros(max(n, 1), np.uint8)
    if n:
        hip = hip_runtime()
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemcpy.restype = C.c_int
        assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), n, 2) == 0  # hipMemcpyDeviceToHost
    return out[:n]


def raw_fetch(eng, n_cap, t_cap):
    """bv_engine_text_tokens_fetch into buffers of the given capacities with sentinels around them: (rc, n, bytes, tokens, text)"""
    from basevar_amd import _capi
    item = _capi.PILEUP_TOKEN_DTYPE.itemsize
    tok = np.full((n_cap + 2) * item, SENTINEL, np.uint8)
    text = np.full(t_cap + 64, SENTINEL, np.uint8)
    n, nb = C.c_uint64(0xDEAD), C.c_uint64(0xDEAD)
    rc = eng._lib.bv_engine_text_tokens_fetch(eng._h, tok.ctypes.data + item, n_cap, text.ctypes.data + 32, t_cap, C.byref(n), C.byref(nb), None)
    assert (tok[:item] == SENTINEL).all() and (tok[(n_cap + 1) * item:] == SENTINEL).all()
    assert (text[:32] == SENTINEL).all() and (text[32 + t_cap:] == SENTINEL).all()
    return rc, int(n.value), int(nb.value), tok[item:(n_cap + 1) * item], text[32:32 + t_cap]


@pytest.mark.parametrize("name", NAMES)
def test_the_list_is_the_models(eng, name):
    """text_tokens_fetch (with sentinels around both buffers) and the device pointers of text_tokens(), against the model; the
    records, row states and planes against the default call; the list is fetched after text_submit"""
    b = batch(name)
    with engine_for(eng, b) as e:
        list_is_the_models(e, b)


def list_is_the_models(eng, b):
    from basevar_amd import _capi
    want = b.tokens()
    exp = lrt_text(eng, b)
    states_are_the_corpus(b, exp)
    got = lrt_text(eng, b, tokens="device")
    same_batch(got, exp)
    assert ttm.tokens_of_arrays(got.tokens, got.token_text) == want
    assert int(got.tokens["text_len"].sum()) == got.token_text.size  # no gaps
    eng.text_tokens_enable(True)
    try:
        same_batch(lrt_text(eng, b), exp)
        n_text = sum(len(t) for p, s, t in want)
        rc, n, nb, tok, text = raw_fetch(eng, len(want), n_text)
        assert (rc, n, nb) == (0, len(want), n_text)
        assert ttm.tokens_of_arrays(np.frombuffer(tok.tobytes(), _capi.PILEUP_TOKEN_DTYPE), text) == want
        (tp, tn), (xp, xn) = eng.text_tokens()
        assert tn == len(want) and (tn == 0) == (tp == 0) and (xn == 0) == (xp == 0)
        dtok = np.frombuffer(device_read(tp, tn * _capi.PILEUP_TOKEN_DTYPE.itemsize).tobytes(), _capi.PILEUP_TOKEN_DTYPE)
        assert ttm.tokens_of_arrays(dtok, device_read(xp, xn)) == want
    finally:
        eng.text_tokens_enable(False)


@pytest.mark.parametrize("name", NAMES)
def test_tally_over_the_device_tokens(eng, name):
    """indel_tally(text_tokens(), key = positions) is indel_string of the host walk's tokens for every position, and
    cvg_format_tallied over it is cvg_format given those columns"""
    b = batch(name)
    with engine_for(eng, b) as e:
        tally_over_the_device_tokens(e, b, name)


def tally_over_the_device_tokens(eng, b, name):
    by_pos = {}
    for p, s, t in b.tokens():
        by_pos.setdefault(p, []).append(t)
    eng.text_tokens_enable(True)
    try:
        got = lrt_text(eng, b)
        key = got.positions
        want = [itr.model_row(by_pos.get(int(p), [])) for p in key]
        tokens, text = eng.text_tokens()
        col_off, flag = eng.indel_tally(key, tokens, text)
        assert flag.tolist() == [w[0] for w in want]
        assert eng.indel_fetch().tobytes() == b"".join(w[1] for w in want)
        assert np.array_equal(np.diff(col_off.astype(np.int64)), [len(w[1]) for w in want])
        if name == "none":
            assert tokens[1] == 0 and not any(w[1] for w in want)
        n = len(key)
        ok = eng.record_text_on_device(got.sites)
        host = [None if ok[k] and not flag[k] else b"row %d left to the host\n" % k for k in range(n)]
        pos, refs = np.arange(100, 100 + n, dtype=np.uint32), b"ACGT" * (n // 4) + b"ACGT"[:n % 4]
        off = eng.cvg_format_tallied(got.sites, b"chrT", pos, refs, host_text=host)
        text_a = eng.cvg_fetch().tobytes()
        want_off = eng.cvg_format(got.sites, b"chrT", pos, refs, indel=[w[1] or None for w in want], host_text=host)
        assert np.array_equal(off, want_off) and text_a == eng.cvg_fetch().tobytes()
        assert text_a or not (got.sites["total_depth"] > 0).any()  # (a record without a covered call gives an empty row)
    finally:
        eng.text_tokens_enable(False)


def members_of(data, member):
    return [bc.member(data[at:at + member], 1) for at in range(0, len(data), member)] + [bc.member(b"")]


@pytest.mark.parametrize("member", [100, 60000])
@pytest.mark.parametrize("name", ["lengths", "states", "lanes", "golden_0"])
def test_bgzf_route_gives_the_text_routes_list(eng, name, member):
    """the same rows as BGZF members (rows span members of 100 bytes): lrt_bgzf(tokens="device") against lrt_text's list and the
    default calls' records; text_heads_fetch against text_rows_fetch with every marked row cut as an unmarked one"""
    from basevar_amd import _capi
    b = batch(name)
    runs = [members_of(b"".join(b.rows[p][f] + b"\n" for p in range(b.P)), member) for f in range(b.F)]
    if member == 100:  # rows span members: file 0's row of some position begins in one member and ends in another
        ends = np.cumsum([len(b.rows[p][0]) + 1 for p in range(b.P)])
        assert any((int(e) - 1) // member != (int(e) - len(b.rows[p][0]) - 1) // member for p, e in enumerate(ends))
    via_text = lrt_text(eng, b, tokens="device")
    exp = eng.lrt_bgzf(runs, b.file_samples, host_reader=ttm.host_reader)
    same_batch(exp, lrt_text(eng, b))
    got = eng.lrt_bgzf(runs, b.file_samples, host_reader=ttm.host_reader, tokens="device")
    same_batch(got, exp)
    assert np.array_equal(got.cursors, exp.cursors)
    assert ttm.tokens_of_arrays(got.tokens, got.token_text) == ttm.tokens_of_arrays(via_text.tokens, via_text.token_text) == b.tokens()
    # the heads: what the rows fetch brought, marked rows of device-parsed positions cut like unmarked ones
    (hbuf, hoff), (rbuf, roff) = got.fetched, exp.fetched
    parse_state = b.parse_state()
    cut = 0
    for p in range(b.P):
        for f in range(b.F):
            r = p * b.F + f
            whole = bytes(rbuf[int(roff[r]):int(roff[r + 1])])
            have = bytes(hbuf[int(hoff[r]):int(hoff[r + 1])])
            if parse_state[p] == 0 and ttm.marked(b.rows[p][f]):
                assert whole == b.rows[p][f]
                assert have == (b"\t".join(whole.split(b"\t")[:4]) + b"\t" if f == 0 else b""), (p, f)
                cut += 1
            else:
                assert have == whole, (p, f)
                assert whole == (b.rows[p][f] if parse_state[p] == ttm.HOST else b"" if parse_state[p] or f else b"\t".join(b.rows[p][f].split(b"\t")[:4]) + b"\t")
    assert cut > 0
    # ... and with the mode on, the rows fetch itself is what it was
    eng.text_tokens_enable(True)
    try:
        again = eng.lrt_bgzf(runs, b.file_samples, host_reader=ttm.host_reader)
        assert again.fetched[0].tobytes() == rbuf.tobytes() and np.array_equal(again.fetched[1], roff)
        assert ttm.tokens_of_arrays(*eng.text_tokens_fetch()) == b.tokens()
    finally:
        eng.text_tokens_enable(False)


def test_the_next_parse_replaces_the_list(eng):
    eng.text_tokens_enable(True)
    try:
        for name in ("lengths", "none", "states", "two_files"):
            b = batch(name)
            lrt_text(eng, b)
            assert ttm.tokens_of_arrays(*eng.text_tokens_fetch()) == b.tokens()
        eng.text_tokens_enable(False)
        lrt_text(eng, batch("only"))  # a parse with the mode off: the list of the parse before it is gone, none takes its place
        eng.text_tokens_enable(True)
        with pytest.raises(RuntimeError):
            eng.text_tokens()
    finally:
        eng.text_tokens_enable(False)


def test_chunks_run_on_from_one_another():
    """An engine of its own, so that the `chunks` batch really is cut (Batch.chunks: five chunks of two positions): the store is
    moved while it holds the chunks before, a later chunk's text does not begin at the text's first byte and its rows not at
    row 0, and the same engine then takes the batch whole -- after a larger one has grown its stage -- with the same list"""
    b = batch("chunks")
    assert b.chunks() == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 9)]
    with engine_for(None, b) as e:
        e.text_tokens_enable(True)
        for _ in range(2):  # (the second time the store has its size already: nothing moves)
            lrt_text(e, b)
            assert ttm.tokens_of_arrays(*e.text_tokens_fetch()) == b.tokens()
        big = batch("lengths")
        lrt_text(e, big)
        assert ttm.tokens_of_arrays(*e.text_tokens_fetch()) == big.tokens()
        lrt_text(e, b)  # one chunk now
        assert ttm.tokens_of_arrays(*e.text_tokens_fetch()) == b.tokens()


def test_heads_fetch_wants_the_token_list(eng):
    """after a parse that listed no tokens the heads would leave the marked rows' tokens nowhere: refused, nothing written, and
    the rows fetch still answers"""
    from basevar_amd import _capi
    b = batch("two_files")
    runs = [members_of(b"".join(b.rows[p][f] + b"\n" for p in range(b.P)), 60000) for f in range(b.F)]
    got = eng.lrt_bgzf(runs, b.file_samples, host_reader=ttm.host_reader)  # the mode is off
    roff, need = np.full(b.P * b.F + 1, 7, np.uint64), C.c_uint64(7)
    for on in (False, True):  # off; on, but the parse was made without it
        eng.text_tokens_enable(on)
        try:
            assert eng._lib.bv_engine_text_heads_fetch(eng._h, None, 0, roff.ctypes.data, C.byref(need), None) == _capi.BV_ERR_INVALID_ARG
            assert need.value == 7 and (roff == 7).all()
        finally:
            eng.text_tokens_enable(False)
    buf, off = eng.text_rows_fetch(b.P * b.F)
    assert buf.tobytes() == got.fetched[0].tobytes() and np.array_equal(off, got.fetched[1])


def test_refusals_leave_the_last_list(eng):
    import basevar_amd as bv
    from basevar_amd import _capi
    INVALID = _capi.BV_ERR_INVALID_ARG
    lib = eng._lib
    T = _capi.IndelTokens()
    n, nb = C.c_uint64(0), C.c_uint64(0)
    fresh = bv.BaseTypeEngine(max_sites=8, min_af_value=bv.min_af(64), device=0, max_samples=64)
    try:
        T.n_tokens = 77
        assert lib.bv_engine_text_tokens(fresh._h, C.byref(T)) == INVALID and T.n_tokens == 77      # the mode is off
        assert lib.bv_engine_text_tokens_enable(fresh._h, 1) == 0
        assert lib.bv_engine_text_tokens(fresh._h, C.byref(T)) == INVALID and T.n_tokens == 77      # no parse
        assert lib.bv_engine_text_tokens_fetch(fresh._h, None, 0, None, 0, C.byref(n), C.byref(nb), None) == INVALID
        roff = np.zeros(4, np.uint64)
        assert lib.bv_engine_text_heads_fetch(fresh._h, None, 0, roff.ctypes.data, C.byref(n), None) == INVALID  # no _parse_bgzf
    finally:
        fresh.close()
    assert lib.bv_engine_text_tokens_enable(None, 1) == INVALID
    b = batch("lengths")
    want = b.tokens()
    n_text = sum(len(t) for p, s, t in want)
    eng.text_tokens_enable(True)
    try:
        lrt_text(eng, b)
        usable = lambda: ttm.tokens_of_arrays(*eng.text_tokens_fetch()) == want  # noqa: E731
        assert usable()
        assert lib.bv_engine_text_tokens(eng._h, None) == INVALID and lib.bv_engine_text_tokens(None, C.byref(T)) == INVALID
        assert lib.bv_engine_text_tokens_fetch(eng._h, None, 0, None, 0, None, C.byref(nb), None) == INVALID
        assert lib.bv_engine_text_tokens_fetch(eng._h, None, 0, None, 0, C.byref(n), None, None) == INVALID
        assert usable()
        for n_cap, t_cap in ((len(want) - 1, n_text), (len(want), n_text - 1), (0, 0)):  # the sizes are written and nothing else
            rc, got_n, got_nb, tok, text = raw_fetch(eng, n_cap, t_cap)
            assert (rc, got_n, got_nb) == (INVALID, len(want), n_text)
            assert (tok == SENTINEL).all() and (text == SENTINEL).all()
        assert usable()
        eng.text_tokens_enable(False)
        assert lib.bv_engine_text_tokens(eng._h, C.byref(T)) == INVALID
        rc, got_n, got_nb, tok, text = raw_fetch(eng, len(want), n_text)
        assert rc == INVALID and (tok == SENTINEL).all()
        eng.text_tokens_enable(True)
        assert usable()
        assert lib.bv_engine_text_tokens(eng._h, C.byref(T)) == 0 and T.n_tokens == len(want) and T.text_bytes == n_text and T.mem_kind == _capi.BV_MEM_DEVICE
    finally:
        eng.text_tokens_enable(False)
