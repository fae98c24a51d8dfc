"""GPU tests of bv_engine_indel_tally, bv_engine_indel_fetch and bv_engine_cvg_format_tallied (include/basevar_amd_indel.h): the
columns, offsets and flags the device gives over the corpus of tests/indel_tally_ref.py are, byte for byte, those of
host/vcf_emit.hpp's indel_string -- printed by the stand-alone harness tests/cpp/indel_tally_check.cpp -- and of the serial
model, from host tokens, from device tokens and from the tokens a pileup left on the engine; the CVG rows around them are
bv_engine_cvg_format's given the model's columns as text; every refusal returns its status and leaves the last tally usable."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import indel_tally_ref as ref  # noqa: E402
import record_text_ref as rt  # noqa: E402

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def harness():
    return ref.build()


@pytest.fixture(scope="module")
def eng():
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(2048), device=0, max_samples=2048)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(harness, tmp_path_factory):
    """the corpus, the harness's dump and the model's rows: computed once, left unchanged"""
    rows = ref.corpus()
    dump = ref.run_rows(harness, rows, tmp_path_factory.mktemp("indel_tally"))
    want = rows.expected()
    assert [(d[0], d[4]) for d in dump] == want
    return rows, want


def offsets(columns):
    off = np.zeros(len(columns) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in columns])
    return off


def on_device(rows, shift=0):
    """the tokens and the text in device memory, the text `shift` bytes into a buffer with sentinels around it"""
    import torch
    tok = rows.tokens
    text = np.full(shift + rows.text.size + 64, SENTINEL, np.uint8)
    text[shift:shift + rows.text.size] = rows.text
    tt = torch.from_numpy(np.frombuffer(tok.tobytes(), np.uint8).copy()).cuda()
    tx = torch.from_numpy(text).cuda()
    torch.cuda.synchronize()
    return (int(tt.data_ptr()), len(tok)), (int(tx.data_ptr()) + shift, int(rows.text.size)), (tt, tx)


def check_tally(eng, rows, want, tokens, text):
    import torch
    col_off, flag = eng.indel_tally(rows.keys, tokens, text)
    assert np.array_equal(flag, [w[0] for w in want])
    assert np.array_equal(col_off, offsets([w[1] for w in want]))
    joined = b"".join(w[1] for w in want)
    assert eng.indel_fetch().tobytes() == joined
    buf = torch.full((len(joined) + 64,), SENTINEL, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert eng.indel_fetch(dst_ptr=int(buf.data_ptr()) + 32, dst_capacity=len(joined)) is None
    got = buf.cpu().numpy()
    assert (got[:32] == SENTINEL).all() and (got[32 + len(joined):] == SENTINEL).all() and got[32:32 + len(joined)].tobytes() == joined


@pytest.mark.parametrize("where", ["host", "device"])
def test_corpus_columns_offsets_and_flags(eng, corpus, where):
    rows, want = corpus
    assert sum(w[0] for w in want) >= 4 and sum(1 for w in want if w[1]) > 60
    if where == "host":
        check_tally(eng, rows, want, rows.tokens, rows.text)
    else:
        tokens, text, keep = on_device(rows, shift=5)
        check_tally(eng, rows, want, tokens, text)
        tt, tx = keep
        back = tx.cpu().numpy()
        assert (back[:5] == SENTINEL).all() and (back[5 + rows.text.size:] == SENTINEL).all() and back[5:5 + rows.text.size].tobytes() == rows.text.tobytes()


def test_shifted_text_gives_the_same_columns(eng, harness, tmp_path):
    """the whole layout moved by 1 .. 15 bytes: every token at every alignment"""
    small = ref.corpus()
    keep_names = [n for n in small.names if not n.startswith(("size_163", "count", "column_"))]
    for lead in (1, 7, 15):
        shifted = ref.corpus(lead)
        keys = [shifted.names[n] for n in keep_names]
        rows = ref.Rows([(p, shifted.rows[p]) for p in keys], keys, lead)
        check_tally(eng, rows, rows.expected(), rows.tokens, rows.text)


def tallied_lines(eng, harness, tmp_path, n, n_groups, device_records=False):
    """cvg_format_tallied over n seeded lines against cvg_format handed the model's columns as text; lines the predicate refuses
    and lines 1 and 62 go as host text, and line 3 is a row beyond the tally's limit, flagged, that brings host text"""
    from test_gpu_record_text import arrays, names_of, on_device_memory
    lines = rt.seeded_lines(7000 + n, n, n_groups, chrom=b"chr5")
    for k, ln in enumerate(lines):
        ln["rec"]["total_depth"] = max(int(ln["rec"]["total_depth"]), 1) if k < 5 else ln["rec"]["total_depth"]
        if k % 9 == 2:
            ln["tokens"] = [b"+AT", b"-C", b"+AT", b"+A\x80", b"+", b"-GGT"][:1 + k % 6] * (1 + k % 4)
    if n > 3:
        lines[3]["tokens"] = ref.cycle([b"+A", b"-T"], ref.LIMIT + 1)
    names = names_of(n_groups)
    dump = rt.run_lines(harness_rt(), lines, names, tmp_path)
    rows = ref.lines_tokens(lines)
    want = rows.expected()
    col_off, flag = eng.indel_tally(rows.keys, rows.tokens, rows.text)
    assert np.array_equal(col_off, offsets([w[1] for w in want])) and np.array_equal(flag, [w[0] for w in want])
    assert n <= 3 or flag[3] == 1
    as_host = [(not d[0]) or k in (1, 62) or bool(flag[k]) for k, d in enumerate(dump)]
    host = [d[3] if h else None for d, h in zip(dump, as_host)]
    sites, groups, pos, refs = arrays(lines, n_groups)
    keep = None
    if device_records:
        sites, groups, keep = on_device_memory(sites, groups)
    off = eng.cvg_format_tallied(sites, b"chr5", pos, refs, host_text=host, groups=groups, group_names=names)
    got = eng.cvg_fetch().tobytes()
    want_off = eng.cvg_format(sites, b"chr5", pos, refs, indel=[w[1] or None for w in want], host_text=host, groups=groups, group_names=names)
    assert np.array_equal(off, want_off) and got == eng.cvg_fetch().tobytes() == b"".join(d[3] for d in dump)
    assert any(w[1] for w in want) or n < 3
    del keep


_RT = []


def harness_rt():
    if not _RT:
        _RT.append(rt.build())
    return _RT[0]


@pytest.mark.parametrize("n_groups", [0, 2])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_cvg_format_tallied_is_cvg_format_with_the_models_columns(eng, harness, tmp_path, n, n_groups):
    tallied_lines(eng, harness, tmp_path, n, n_groups, device_records=(n == 65))


def tally_of_the_pileup(eng, harness, tmp_path, window):
    """tok == NULL: the columns of every position of the window against indel_string over the fetched tokens"""
    got = eng.pileup_fetch()
    keys = list(range(window[0], window[1] + 1))
    rows = ref.Rows.from_arrays(got["tokens"], got["text"], keys + keys[::-1][:3])
    dump = ref.run_rows(harness, rows, tmp_path)
    want = rows.expected()
    assert [(d[0], d[4]) for d in dump] == want
    col_off, flag = eng.indel_tally(rows.keys)
    assert np.array_equal(flag, [w[0] for w in want]) and np.array_equal(col_off, offsets([w[1] for w in want]))
    assert eng.indel_fetch().tobytes() == b"".join(w[1] for w in want)
    return sum(1 for w in want if w[1])


def test_tokens_of_a_pileup_of_bam_files_and_of_their_members(harness, tmp_path):
    import bam_members as bm
    import pileup_ref as pr
    from test_gpu_pileup_bgzf import engine
    c = bm.Corpus(tmp_path / "corpus", 65, 700, True)
    w = pr.WINDOWS["w1000"]
    d, p, _ = bm.run_plan(bm.build(), tmp_path / "plan.bin", c.fasta, c.bams[:65], w)
    e = engine(c.fa, n=65)
    try:
        e.pileup(d.records, d.run_off, d.run_sample, 65, d.tid, pr.REGION, w, pr.MAPQ_THD)
        n_a = tally_of_the_pileup(e, harness, tmp_path, w)
        text_a = e.indel_fetch().tobytes()
        e.pileup_bgzf(p.data, p.member_off, p.runs, 65, d.tid, pr.REGION, w, pr.MAPQ_THD)
        n_b = tally_of_the_pileup(e, harness, tmp_path, w)
        assert n_a == n_b >= 3 and e.indel_fetch().tobytes() == text_a
    finally:
        e.close()


def test_tokens_of_the_hand_built_raw_cases(harness, tmp_path):
    import pileup_raw_cases as rc
    import pileup_ref as pr
    from test_gpu_pileup import engine
    e = engine(None, n=130)
    try:
        with_columns = 0
        cases = [c for _, c in sorted(rc.directed().items()) if not c.status]
        cases = [(c.tuple(), c.ref) for c in cases] + [(rc.campaign_round(s), None) for s in rc.CAMPAIGN_SEEDS[:4]]
        for case, fa in cases:
            runs, run_sample, n, window, cref = case
            e.pileup_set_reference(fa if fa is not None else cref)
            off = np.zeros(len(runs) + 1, np.uint64)
            off[1:] = np.cumsum([len(r) for r in runs])
            e.pileup(np.frombuffer(b"".join(runs), np.uint8), off, run_sample, n, pr.TID, pr.REGION, window, pr.MAPQ_THD)
            with_columns += tally_of_the_pileup(e, harness, tmp_path, window)
        assert with_columns >= 10
    finally:
        e.close()


def test_refusals_leave_the_last_tally(eng, corpus):
    import torch
    from basevar_amd import _capi
    rows = ref.Rows([(10, [b"+A", b"-C", b"+A"]), (12, [b"-GG"])], [12, 10, 11])
    want = [b"-GG|1", b"+A|2,-C|1", b""]
    lib, h = eng._lib, eng._h
    col_off, flag = np.zeros(4, np.uint64), np.zeros(3, np.uint8)

    def still_held():
        assert eng.indel_fetch().tobytes() == b"".join(want)
        sites = np.zeros(3, _capi.SITE_DTYPE)
        sites["total_depth"] = 7
        eng.cvg_format_tallied(sites, b"c", np.array([12, 10, 11], np.uint32), b"ACG")
        assert [ln.split(b"\t")[8] for ln in eng.cvg_fetch().tobytes().splitlines()] == [w or b"." for w in want]

    def raw(tok, key=rows.keys, n=3, out=col_off, flags=flag):
        col_off[:] = 7
        rc = lib.bv_engine_indel_tally(h, C.byref(tok) if tok is not None else None, key.ctypes.data if key is not None else None, n,
                                       out.ctypes.data if out is not None else None, flags.ctypes.data if flags is not None else None, None)
        assert rc == _capi.BV_OK or (col_off == 7).all()  # a refusal leaves it unwritten
        return rc

    def tokens(**change):
        T = _capi.IndelTokens(rows.tokens.ctypes.data, rows.text.ctypes.data, len(rows.tokens), rows.text.size, _capi.BV_MEM_HOST, 0)
        for k, v in change.items():
            setattr(T, k, v)
        return T

    got_off, got_flag = eng.indel_tally(rows.keys, rows.tokens, rows.text)
    assert np.array_equal(got_off, offsets(want)) and not got_flag.any()
    still_held()
    INVALID = _capi.BV_ERR_INVALID_ARG
    assert raw(tokens(), key=None) == INVALID and raw(tokens(), out=None) == INVALID and raw(tokens(), flags=None) == INVALID
    assert raw(tokens(reserved_=1)) == INVALID and raw(tokens(mem_kind=2)) == INVALID
    assert raw(tokens(tokens=None)) == INVALID and raw(tokens(text=None)) == INVALID
    assert raw(None) == INVALID and b"no completed bv_engine_pileup" in lib.bv_last_error(h)  # (this engine has piled nothing up)
    down = rows.tokens.copy()
    down["pos"][-1] = 5
    assert raw(tokens(tokens=down.ctypes.data)) == INVALID and b"pos descends" in lib.bv_last_error(h)
    beyond = rows.tokens.copy()
    beyond["text_len"][1] = rows.text.size
    assert raw(tokens(tokens=beyond.ctypes.data)) == INVALID and b"beyond text_bytes" in lib.bv_last_error(h)
    assert raw(tokens(text_bytes=rows.text.size - 1)) == INVALID
    still_held()
    # the same damage in device memory: found by the first kernel, nothing written
    for bad in (down, beyond):
        tt = torch.from_numpy(np.frombuffer(bad.tobytes(), np.uint8).copy()).cuda()
        tx = torch.from_numpy(rows.text.copy()).cuda()
        torch.cuda.synchronize()
        assert raw(tokens(tokens=int(tt.data_ptr()), text=int(tx.data_ptr()), mem_kind=_capi.BV_MEM_DEVICE)) == INVALID
        still_held()
    # cvg_format_tallied's own refusals
    sites = np.zeros(3, _capi.SITE_DTYPE)
    sites["total_depth"] = 7
    pos = np.array([12, 10, 11], np.uint32)
    L, keep, texts = eng._record_lines("test", sites, None, b"c", pos, b"ACG", (), None, 3)
    L.indel_off, L.indel = texts([b"+A|1", None, None])
    line_off = np.zeros(4, np.uint64)
    assert lib.bv_engine_cvg_format_tallied(h, C.byref(L), line_off.ctypes.data, None) == INVALID
    with pytest.raises(RuntimeError, match="the last tally has 3 rows") as ei:
        eng.cvg_format_tallied(sites[:2], b"c", pos[:2], b"AC")
    assert ei.value.args[1] == INVALID
    still_held()
    # a flagged row that brings no host text; and with it
    big = ref.Rows([(1, ref.cycle([b"+A"], ref.LIMIT + 1))], [1, 2, 1])
    _, f = eng.indel_tally(big.keys, big.tokens, big.text)
    assert list(f) == [1, 0, 1]
    with pytest.raises(RuntimeError, match="line 0: the tally left its indel column to the caller") as ei:
        eng.cvg_format_tallied(sites, b"c", pos, b"ACG")
    assert ei.value.args[1] == INVALID
    eng.cvg_format_tallied(sites, b"c", pos, b"ACG", host_text=[b"row0\n", None, b"row2\n"])
    assert eng.cvg_fetch().tobytes().startswith(b"row0\nc\t10\tC\t7\t0\t0\t0\t0\t.\t") and eng.cvg_fetch().tobytes().endswith(b"row2\n")
    # no rows: BV_OK, col_off[0] = 0, and a fresh engine has no tally
    off0, _ = eng.indel_tally(np.zeros(0, np.uint32), rows.tokens, rows.text)
    assert np.array_equal(off0, [0]) and eng.indel_fetch().size == 0
    import basevar_amd as bv
    fresh = bv.BaseTypeEngine(max_sites=8, min_af_value=bv.min_af(8), device=0, max_samples=8)
    try:
        with pytest.raises(RuntimeError, match="no bv_engine_indel_tally before it"):
            fresh.cvg_format_tallied(sites, b"c", pos, b"ACG")
        buf = np.zeros(16, np.uint8)
        assert lib.bv_engine_indel_fetch(fresh._h, buf.ctypes.data, 16, _capi.BV_MEM_HOST, None) == INVALID
    finally:
        fresh.close()
