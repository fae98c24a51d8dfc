"""GPU tests of bv_engine_text_parse_bgzf_region (include/basevar_amd_region.h): lrt_bgzf(region=...) takes the rows that the
serial model tests/text_region_model.py selects from the files' bytes -- the number of positions, the cursors and region_done
are the model's -- and gives on them what lrt_text gives on the same rows uncompressed (records, row_state, cell / phred), and
what a plain lrt_bgzf gives on files that hold those rows alone (the fetched text, the tokens)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import text_region_model as trm  # noqa: E402
from test_gpu_bgzf_rows import FS3, HEAD, TILE, check_fetched, cursor_of, engine, fit_newline, members_of, pad_row, plain_rows, same_batch  # noqa: E402

CHR = b"chr7"  # pad_row's contig


def on_contig(rows, chrom):
    return [chrom + r[len(CHR):] for r in rows]


def three_contigs(n, salt, before=6, inside=40, behind=5, first=100):
    """rows of n samples: chr6, then chr7 at POS first .. first + inside - 1, then chr8"""
    return (on_contig(plain_rows(before, n, salt, 1), b"chr6") + plain_rows(inside, n, salt, first) + on_contig(plain_rows(behind, n, salt, 1), b"chr8"))


def member_sizes(text, member):
    return [min(member, len(text) - at) for at in range(0, len(text), member)] + [0]


def region_check(eng, texts, fs, region, skip_bytes=None, skip_lines=None, at_end=True, max_positions=None, member=0x5000, tokens="host", want_positions=None):
    """lrt_bgzf(region=...) on the files' texts against the model and, through lrt_text and a plain lrt_bgzf on the selected rows,
    against the rest of the engine.  Returns (got, the model's answer)."""
    F = len(fs)
    member = member if isinstance(member, (list, tuple)) else [member] * F
    sb = list(skip_bytes) if skip_bytes is not None else [0] * F
    sl = list(skip_lines) if skip_lines is not None else [0] * F
    exp = trm.select(texts, region, sb, sl, at_end, max_positions, eng.max_sites)
    assert exp["err"] is None, exp["err"]
    P = exp["P"]
    if want_positions is not None:
        assert P == want_positions, (P, want_positions)
    runs = [members_of(t, m) for t, m in zip(texts, member)]
    got = eng.lrt_bgzf(runs, fs, skip_bytes=sb, skip_lines=sl, at_end=at_end, max_positions=max_positions, tokens=tokens, region=region)
    assert got.row_state.shape == (P, F), (got.row_state.shape, P)
    assert got.cursors.tolist() == [cursor_of(member_sizes(texts[f], member[f]), exp["cursor"][f]) for f in range(F)], (got.cursors.tolist(), exp["cursor"])
    assert got.region_done == exp["done"]
    if P == 0:
        assert len(got.sites) == 0 and got.fetched[0].size == 0
        return got, exp
    rows = [[texts[f][a:b] for f, (a, b) in enumerate(r)] for r in exp["rows"]]
    ref = eng.lrt_text(rows, fs, tokens=tokens)  # (raises if a position is not in the strict form)
    same_batch(got, ref, 0)
    alone = eng.lrt_bgzf([members_of(b"".join(rows[p][f] + b"\n" for p in range(P)), 0x3000) for f in range(F)], fs, tokens=tokens)
    same_batch(got, alone, 0)
    assert got.fetched[0].tobytes() == alone.fetched[0].tobytes() and np.array_equal(got.fetched[1], alone.fetched[1])
    if tokens == "device":
        for other in (ref, alone):
            assert got.tokens.tobytes() == other.tokens.tobytes() and got.token_text.tobytes() == other.token_text.tobytes()
    else:
        flat = np.frombuffer(b"".join(r + b"\n" for pos in rows for r in pos), np.uint8)
        off = np.concatenate([[0], np.cumsum([len(r) + 1 for pos in rows for r in pos])]).astype(np.uint64)
        check_fetched(got, flat, off, P, F)
    return got, exp


@pytest.mark.parametrize("fs", [[1], [63, 64], [65, 200, 1]])
def test_a_region_in_the_middle_of_three_contigs(fs):
    """files of 1, 63, 64, 65 and 200 samples, one to three files, headers in some: the region's rows out of the middle contig;
    in the file of 200 samples more than one 16 KiB tile of skipped lines lies in front of them"""
    F = len(fs)
    heads = [HEAD[f] if f % 2 == 0 else b"" for f in range(F)]
    texts = [heads[f] + b"".join(three_contigs(fs[f], f, before=6 + f)) for f in range(F)]
    eng = engine(64, sum(fs))
    try:
        got, exp = region_check(eng, texts, fs, (CHR, 115, 127), skip_lines=[1 if h else 0 for h in heads], want_positions=13)
        assert [x["first"] for x in exp["files"]] == [6 + f + 15 for f in range(F)] and exp["done"]
        if 200 in fs:
            f = fs.index(200)
            assert exp["rows"][0][f][0] > 2 * TILE
        assert got.n_variant >= 0 and len(got.sites) == 13
        # the whole contig, open-ended as a reader of CHR or CHR:BEG asks for it; nothing before it, nothing behind it
        region_check(eng, texts, fs, (CHR, 1, 1 << 29), skip_lines=[1 if h else 0 for h in heads], want_positions=40)
        region_check(eng, texts, fs, (b"chr6", 3, 6), skip_lines=[1 if h else 0 for h in heads], want_positions=4)
        region_check(eng, texts, fs, (b"chr8", 1, 2), skip_lines=[1 if h else 0 for h in heads], want_positions=2)
        # names that are a proper prefix or extension of the lines' CHROM select nothing and consume everything
        for name in (b"chr", b"chr77"):
            got, exp = region_check(eng, texts, fs, (name, 1, 1 << 29), skip_lines=[1 if h else 0 for h in heads], want_positions=0)
            assert exp["cursor"] == [len(t) for t in texts] and exp["done"]
    finally:
        eng.close()


def test_heads_that_cross_a_tile_edge():
    """a line that begins on the last byte of a 16 KiB tile, on the first byte of the next, and four bytes before the edge (its
    CHROM spans it) -- as the region's first row, as a row inside it and as the line that ends it; in file 0 and in the last file"""
    P, F = 90, 3
    eng = engine(128, sum(FS3))
    try:
        for at in (TILE - 2, TILE - 1, TILE - 5, 2 * TILE - 2, 2 * TILE - 1):
            texts, hit = [], []
            for f in range(F):
                rows = plain_rows(P, FS3[f], f)
                if f != 1:
                    rows, j = fit_newline(rows, FS3[f], f, at)
                    hit.append(j)
                texts.append(b"".join(rows))
            assert hit[0] + 1 < P and hit[1] + 1 < P
            for f, j in ((0, hit[0]), (2, hit[1])):
                pos = j + 2  # POS of the row that begins at byte at + 1 (row j + 1; POS = row index + 1)
                assert texts[f][at] == 10 and texts[f][at + 1:].startswith(b"chr7\t%d\t" % pos)
                got, exp = region_check(eng, texts, FS3, (CHR, pos, pos + 5), want_positions=6)
                assert exp["rows"][0][f][0] == at + 1
                got, exp = region_check(eng, texts, FS3, (CHR, pos - 3, pos + 3), want_positions=7)
                assert exp["rows"][3][f][0] == at + 1
                got, exp = region_check(eng, texts, FS3, (CHR, pos - 4, pos - 1), want_positions=4)
                assert exp["cursor"][f] == at + 1 and exp["done"]
    finally:
        eng.close()


def test_a_line_start_on_every_lane():
    """rows of 64 consecutive lengths, twice: read back from the built bytes, the line breaks in front of the region's rows fall on
    each of the 64 lanes, behind a skip that is no multiple of 64"""
    P, n = 140, 40
    rows = [pad_row(1 + p, n, 0, 450 + p % 64) for p in range(P)]
    text0 = HEAD[0] + b"".join(rows)
    eng = engine(P, n + 20)
    try:
        got, exp = region_check(eng, [text0, b"".join(plain_rows(P, 20, 1))], [n, 20], (CHR, 5, 135), skip_bytes=[len(HEAD[0]), 0], want_positions=131)
        lanes = {(r[0][0] - 1 - len(HEAD[0])) % 64 for r in exp["rows"]}
        assert lanes == set(range(64)) and all(text0[r[0][0] - 1] == 10 for r in exp["rows"])
    finally:
        eng.close()


def test_files_whose_members_differ():
    """the same rows in members of 100 and of 60,000 bytes, and of 0x1000 behind header lines: the same line lies at different
    offsets of different members, and the cursors name them"""
    fs = [60, 60, 60]
    texts = [b"".join(three_contigs(60, 0)), b"".join(three_contigs(60, 0)), HEAD[2] + b"".join(three_contigs(60, 0))]
    eng = engine(64, sum(fs))
    try:
        got, exp = region_check(eng, texts, fs, (CHR, 110, 119), skip_lines=[0, 0, 1], member=[100, 60000, 0x1000], max_positions=7, want_positions=7)
        assert not exp["done"] and got.cursors[0, 0] > 50 and got.cursors[1, 0] == 0 and got.cursors[1, 1] == exp["cursor"][1]
    finally:
        eng.close()


def chained(eng, texts, fs, region, headers, members, window, at_end_from=0):
    """the region taken `window` positions at a time, every run starting at the member the last cursor names, until
    region_done; returns the batches.  A file whose cursor moved has its header lines behind it."""
    F = len(fs)
    files = [members_of(t, m) for t, m in zip(texts, members)]
    starts = [np.concatenate([[0], np.cumsum(member_sizes(t, m))]) for t, m in zip(texts, members)]
    at, skip_b, skip_l = [0] * F, [0] * F, list(headers)
    parts = []
    for _ in range(400):
        x = [int(starts[f][at[f]]) + skip_b[f] for f in range(F)]
        exp = trm.select(texts, region, x, skip_l, True, window, eng.max_sites)
        got = eng.lrt_bgzf([files[f][at[f]:] for f in range(F)], fs, skip_bytes=skip_b, skip_lines=skip_l, max_positions=window, region=region)
        assert got.row_state.shape[0] == exp["P"] and got.region_done == exp["done"]
        parts.append(got)
        for f in range(F):
            moved = got.cursors[f].tolist() != cursor_of(member_sizes(texts[f], members[f])[at[f]:], skip_b[f])
            at[f] += int(got.cursors[f, 0])
            skip_b[f] = int(got.cursors[f, 1])
            assert int(starts[f][min(at[f], len(starts[f]) - 1)]) + skip_b[f] == exp["cursor"][f]
            if moved:
                skip_l[f] = 0
        if got.region_done:
            return parts
    raise AssertionError("the region never ended")


@pytest.mark.parametrize("window", [1, 7, "tile"])
def test_regions_chained_through_the_cursors(window):
    """max_positions 1, 7 and the count that ends a window with a row whose line break is the last byte of a tile: the windows
    together are the region taken at once"""
    fs = FS3
    P, F = 90, 3
    rows0, hit = fit_newline(plain_rows(P, fs[0], 0), fs[0], 0, TILE - 1)
    texts = [b"".join(rows0), HEAD[1] + HEAD[1] + b"".join(plain_rows(P, fs[1], 1)), b"".join(on_contig(plain_rows(4, fs[2], 2), b"chr6") + plain_rows(P, fs[2], 2))]
    first_pos = 8
    region = (CHR, first_pos, 80)
    if window == "tile":
        window = hit + 1 - (first_pos - 1)  # rows first_pos - 1 .. hit of file 0
        assert texts[0][TILE - 1] == 10 and window > 7
    eng = engine(128, sum(fs))
    try:
        whole, exp = region_check(eng, texts, fs, region, skip_lines=[0, 2, 0], want_positions=73)
        parts = chained(eng, texts, fs, region, [0, 2, 0], [0x1000, 0x100, 0xff00], window)
    finally:
        eng.close()
    assert [p.row_state.shape[0] for p in parts] == [window] * (73 // window) + ([73 % window] if 73 % window else [])
    assert np.array_equal(np.concatenate([p.row_state for p in parts]), whole.row_state)
    assert b"".join(p.sites.tobytes() for p in parts) == whole.sites.tobytes()
    assert b"".join(p.cell.tobytes() for p in parts) == whole.cell.tobytes() and b"".join(p.phred.tobytes() for p in parts) == whole.phred.tobytes()


def test_regions_without_rows_and_regions_that_end_with_the_file():
    fs = [40, 24]
    gap = [plain_rows(10, n, s, 1) + plain_rows(10, n, s, 50) for s, n in enumerate(fs)]
    texts = [b"".join(r) for r in gap]
    eng = engine(64, sum(fs))
    try:
        # between two lines: no row, done at once (the line at POS 50 ends it), the lines in front are consumed
        got, exp = region_check(eng, texts, fs, (CHR, 20, 40), at_end=False, want_positions=0)
        assert exp["done"] and [x["first"] for x in exp["files"]] == [10, 10] and exp["cursor"] == [len(b"".join(r[:10])) for r in gap]
        # before all lines: done at once, nothing consumed
        got, exp = region_check(eng, on_contig_texts(gap, 5), fs, (CHR, 1, 4), at_end=False, want_positions=0)
        assert exp["done"] and exp["cursor"] == [0, 0]
        # behind all lines: only the end of the files ends it
        got, exp = region_check(eng, texts, fs, (CHR, 100, 200), at_end=False, want_positions=0)
        assert not exp["done"] and exp["cursor"] == [len(t) for t in texts]
        got, exp = region_check(eng, texts, fs, (CHR, 100, 200), at_end=True, want_positions=0)
        assert exp["done"]
        # rows up to the last line: done only with at_end; the call behind it has nothing left and says so
        got, exp = region_check(eng, texts, fs, (CHR, 55, 200), at_end=False, want_positions=5)
        assert not exp["done"] and exp["cursor"] == [len(t) for t in texts]
        got, exp = region_check(eng, texts, fs, (CHR, 55, 200), at_end=True, want_positions=5)
        assert exp["done"]
        got, exp = region_check(eng, texts, fs, (CHR, 55, 200), skip_bytes=[len(t) for t in texts], at_end=True, want_positions=0)
        assert exp["done"] and got.cursors.tolist() == [[2, 0], [2, 0]]  # (behind the member with the text and the empty last one)
        # a last line without a line break is a row with at_end, and no line without
        cut = [t[:-1] for t in texts]
        region_check(eng, cut, fs, (CHR, 55, 200), at_end=True, want_positions=5)
        got, exp = region_check(eng, cut, fs, (CHR, 55, 200), at_end=False, want_positions=4)
        assert not exp["done"]
    finally:
        eng.close()


def on_contig_texts(rows_per_file, shift):
    """the files' rows with POS moved up by `shift`: rebuilt, so that every row stays well-formed"""
    out = []
    for rows in rows_per_file:
        moved = []
        for r in rows:
            c = r.split(b"\t", 2)
            moved.append(c[0] + b"\t%d\t" % (int(c[1]) + shift) + c[2])
        out.append(b"".join(moved))
    return out


def test_tokens_on_the_device_and_the_heads_behind_a_region():
    """tokens="device": the list and text_heads_fetch are those of the same rows parsed alone; the region's rows hold insertion
    tokens (pad_row with a length) in front of, at and behind the region's edges"""
    fs = [40, 24]
    rows = [[pad_row(1 + p, n, s, 600 + 3 * p) if p % 3 == 0 else pad_row(1 + p, n, s) for p in range(60)] for s, n in enumerate(fs)]
    texts = [b"".join(r) for r in rows]
    eng = engine(64, sum(fs))
    try:
        got, exp = region_check(eng, texts, fs, (CHR, 10, 40), tokens="device", want_positions=31)
        assert len(got.tokens) >= 2 * 10 and got.token_text.size > 0
        region_check(eng, texts, fs, (CHR, 10, 40), tokens="host", want_positions=31)
    finally:
        eng.close()


def test_refused_data_names_file_and_line():
    """each BV_ERR_DATA case: the message has file and line, nothing was parsed, the engine goes on and the next plain lrt_bgzf
    is what it was"""
    from basevar_amd import _capi
    fs = [40, 24, 30]
    good = [three_contigs(n, s) for s, n in enumerate(fs)]  # chr7 at lines 6 .. 45, POS 100 .. 139
    region = (CHR, 110, 125)

    def texts_with(f, change):
        rows = [list(r) for r in good]
        change(rows[f])
        return [b"".join(r) for r in rows]

    def bad_head(rows):
        rows[6 + 12] = rows[6 + 12].replace(b"\t112\t", b"\t112x\t", 1)

    def bad_head_in_front(rows):
        rows[2] = rows[2].replace(b"\t", b" ", 1)

    def one_row_less(rows):
        del rows[6 + 20]

    def ends_early(rows):
        del rows[6 + 22:]

    def other_pos(rows):
        rows[6 + 14] = pad_row(113, fs[1], 1)

    cases = [(1, bad_head, r"file 1, line 18 behind its skip: the head is not"),
             (2, bad_head_in_front, r"file 2, line 2 behind its skip: the head is not"),
             (1, one_row_less, r"file 1, line 31 behind its skip: the file's lines of the region end here, file 0 has more"),
             (2, ends_early, r"file 2, line 28 behind its skip: the file's lines of the region end here, file 0 has more"),
             (1, other_pos, r"file 1, position 4 of the region's rows \(line 20 behind its skip\): POS differs from file 0's")]
    eng = engine(64, sum(fs))
    try:
        plain_runs = [members_of(b"".join(r), 0x2000) for r in good]
        before = eng.lrt_bgzf(plain_runs, fs)
        for f, change, message in cases:
            texts = texts_with(f, change)
            assert trm.select(texts, region, max_positions=64)["err"] is not None
            with pytest.raises(RuntimeError, match=message) as ei:
                eng.lrt_bgzf([members_of(t, 0x2000) for t in texts], fs, region=region)
            assert ei.value.args[1] == _capi.BV_ERR_DATA and "bv_engine_text_parse_bgzf_region" in ei.value.args[0]
            out = np.zeros(1, dtype=_capi.SITE_DTYPE)  # nothing was parsed: there is nothing to submit or to fetch
            assert eng._lib.bv_engine_text_submit(eng._h, None, None, 1, out.ctypes.data, None, None, None, None) == _capi.BV_ERR_INVALID_ARG
            with pytest.raises(RuntimeError, match="no bv_engine_text_parse_bgzf"):
                eng.text_rows_fetch(3)
            same_batch(eng.lrt_bgzf(plain_runs, fs), before, 0)
            region_check(eng, [b"".join(r) for r in good], fs, region, want_positions=16)
        # what is not looked at: a malformed head behind the line that ends the selection; a POS that differs behind max_positions
        texts = texts_with(1, lambda rows: rows.__setitem__(6 + 30, rows[6 + 30].replace(b"\t", b" ", 1)))
        region_check(eng, texts, fs, region, want_positions=16)
        region_check(eng, texts_with(1, other_pos), fs, region, max_positions=4, want_positions=4)
    finally:
        eng.close()


def raw_call(eng, runs, fs, region, state_ptr, cursor_ptr, done_ptr, max_positions=64, npos_ptr=None):
    from basevar_amd import _capi
    F = len(fs)
    members = [bytes(m) for run in runs for m in run]
    data = np.frombuffer(b"".join(members), dtype=np.uint8)
    moff = np.zeros(len(members) + 1, dtype=np.uint64)
    moff[1:] = np.cumsum([len(m) for m in members])
    fm = np.zeros(F + 1, dtype=np.uint32)
    fm[1:] = np.cumsum([len(run) for run in runs])
    fsa = np.ascontiguousarray(fs, dtype=np.uint32)
    sb, sl = np.zeros(F, np.uint64), np.zeros(F, np.uint32)
    br = _capi.BgzfRows(data.ctypes.data, moff.ctypes.data, int(data.size), fm.ctypes.data, fsa.ctypes.data, sb.ctypes.data, sl.ctypes.data, F, max_positions, 1, 0)
    n_pos = C.c_uint32(0xDEAD)
    rc = eng._lib.bv_engine_text_parse_bgzf_region(eng._h, C.byref(br), C.byref(region) if region is not None else None, None, 0,
                                                   npos_ptr if npos_ptr is not None else C.byref(n_pos), state_ptr, cursor_ptr, done_ptr, None)
    return rc, n_pos.value


def test_argument_refusals_and_sentinels():
    from basevar_amd import _capi
    fs = [40, 24]
    texts = [b"".join(three_contigs(n, s)) for s, n in enumerate(fs)]
    runs = [members_of(t, 0x2000) for t in texts]
    F, P = 2, 16
    eng = engine(64, sum(fs))
    try:
        for bad in ((None, 1, 2), (b"", 1, 2), (CHR, 0, 5), (CHR, 6, 5), (CHR, 1, 5, 1)):
            with pytest.raises(RuntimeError, match=r"bv_engine_text_parse_bgzf_region failed \(-1\)"):
                eng.lrt_bgzf(runs, fs, region=bad)
        for kw in (dict(skip_bytes=[1 << 30, 0]), dict(max_positions=0), dict(file_samples=[0, 24]), dict(file_samples=[41, 24]), dict(n_groups=2)):
            args = dict(runs=runs, file_samples=fs, region=(CHR, 110, 125))
            args.update(kw)
            with pytest.raises(RuntimeError, match=r"bv_engine_text_parse_bgzf_region failed \(-1\)"):
                eng.lrt_bgzf(**args)
        # guarded outputs: row_state is written for P * F rows and the cursors for F files, nothing around them
        state = np.full(64 * F + 128, 0xA5, np.uint8)
        cur = np.full((F + 4, 2), 0x5A5A5A5A, np.uint32)
        done = (C.c_uint32 * 3)(0x77777777, 0x77777777, 0x77777777)
        rg = _capi.TextRegion(CHR, len(CHR), 110, 125, 0)
        done_ptr = C.cast(C.byref(done, 4), C.POINTER(C.c_uint32))
        assert raw_call(eng, runs, fs, None, state.ctypes.data + 64, cur.ctypes.data + 16, done_ptr)[0] == _capi.BV_ERR_INVALID_ARG
        assert raw_call(eng, runs, fs, rg, state.ctypes.data + 64, cur.ctypes.data + 16, None)[0] == _capi.BV_ERR_INVALID_ARG
        assert raw_call(eng, runs, fs, rg, None, cur.ctypes.data + 16, done_ptr)[0] == _capi.BV_ERR_INVALID_ARG
        assert raw_call(eng, runs, fs, rg, state.ctypes.data + 64, None, done_ptr)[0] == _capi.BV_ERR_INVALID_ARG
        assert (state == 0xA5).all() and (cur == 0x5A5A5A5A).all() and list(done) == [0x77777777] * 3
        rc, n = raw_call(eng, runs, fs, rg, state.ctypes.data + 64, cur.ctypes.data + 16, done_ptr)
        assert (rc, n) == (0, P) and list(done) == [0x77777777, 1, 0x77777777]
        assert (state[:64] == 0xA5).all() and (state[64 + P * F:] == 0xA5).all() and not (state[64:64 + P * F] & ~np.uint8(_capi.BV_TEXT_INDEL)).any()
        assert (cur[:2] == 0x5A5A5A5A).all() and (cur[2 + F:] == 0x5A5A5A5A).all()
        exp = trm.select(texts, (CHR, 110, 125), max_positions=64)
        assert cur[2:2 + F].tolist() == [cursor_of(member_sizes(texts[f], 0x2000), exp["cursor"][f]) for f in range(F)]
        out = np.zeros(P, dtype=_capi.SITE_DTYPE)  # the parse stands: its submit runs
        assert eng._lib.bv_engine_text_submit(eng._h, None, None, P, out.ctypes.data, None, None, None, None) == 0
        assert len(eng.lrt_bgzf(runs, fs).sites) > 0
    finally:
        eng.close()
