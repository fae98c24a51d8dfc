"""GPU tests of bv_engine_text_parse_bgzf / bv_engine_text_rows_fetch (include/basevar_amd_bgzf.h): batchfile rows that reach
the engine as BGZF members give what BaseTypeEngine.lrt_text gives on the same rows uncompressed -- which
tests/test_gpu_text_rows.py holds to lrt()."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzf_corpus as bc  # noqa: E402
from basevar_amd.synth import make_slab  # noqa: E402
from test_gpu_text_rows import _py_host_reader, slab_rows  # noqa: E402


def file_texts(text, row_off, P, F, headers=None, last_newline=True):
    """the position-major rows as F file texts (bytes): header lines first, then the file's row of every position"""
    out = []
    for f in range(F):
        rows = [bytes(text[int(row_off[p * F + f]):int(row_off[p * F + f + 1])]) for p in range(P)]
        t = b"".join(([b"##header of file %d line %d\n" % (f, k) for k in range(headers[f])] if headers else []) + rows)
        out.append(t if last_newline else t[:-1])
    return out


def members_of(data, member, level=1):
    """data as BGZF members of `member` bytes of text each, and the empty end-of-file member"""
    return [bc.member(data[at:at + member], level) for at in range(0, len(data), member)] + [bc.member(b"")]


def engine(P, N):
    import basevar_amd as bv
    return bv.BaseTypeEngine(max_sites=P, min_af_value=bv.min_af(N), device=0, max_samples=N)


def same_batch(got, exp, groups):
    assert np.array_equal(got.row_state, exp.row_state)
    assert np.array_equal(got.positions, exp.positions)
    assert got.sites.tobytes() == exp.sites.tobytes()
    if groups:
        assert got.groups.tobytes() == exp.groups.tobytes()
    assert got.n_variant == exp.n_variant
    assert got.cell.tobytes() == exp.cell.tobytes() and got.phred.tobytes() == exp.phred.tobytes()


def compare(slab, fs, n_groups=0, depth_zero=(), member=0xff00, level=1, headers=None, last_newline=True, members_of=members_of):
    from basevar_amd import _capi
    P, N, F = slab["base_strand"].shape[0], int(slab["n_samples"]), len(fs)
    text, row_off = slab_rows(slab, fs, depth_zero)
    gid = slab.get("group_id") if n_groups else None
    eng = engine(P, N)
    try:
        exp = eng.lrt_text((text, row_off), fs, group_id=gid, n_groups=n_groups)
        runs = [members_of(t, member, level) for t in file_texts(text, row_off, P, F, headers, last_newline)]
        got = eng.lrt_bgzf(runs, fs, skip_lines=headers, group_id=gid, n_groups=n_groups)
    finally:
        eng.close()
    assert got.row_state.shape == (P, F)
    assert not (got.row_state & _capi.BV_TEXT_HOST).any(), "a well-formed position went to the host reader"
    same_batch(got, exp, n_groups)
    for f in range(F):  # everything was taken: the cursor is behind the run's last member with text
        assert got.cursors[f].tolist() in ([len(runs[f]) - 1, 0], [len(runs[f]), 0]), (f, got.cursors[f])
    check_fetched(got, text, row_off, P, F)
    return got, exp


def check_fetched(got, text, row_off, P, F, first=0, host_positions=()):
    """the fetched text: CHROM, POS, REF, Depth of file 0's row for every kept position, indel rows whole, nothing else"""
    from basevar_amd import _capi
    buf, roff = got.fetched
    for p in range(got.row_state.shape[0]):
        for f in range(F):
            r = p * F + f
            row = bytes(text[int(row_off[(first + p) * F + f]):int(row_off[(first + p) * F + f + 1]) - 1])
            have = bytes(buf[int(roff[r]):int(roff[r + 1])])
            s = int(got.row_state[p, f])
            if p in host_positions:  # (whatever the host reader made of it afterwards)
                assert have == row, (p, f)
            elif s & _capi.BV_TEXT_SKIP:
                assert have == b""
            elif s & (_capi.BV_TEXT_HOST | _capi.BV_TEXT_INDEL):
                assert have == row, (p, f)
            elif f == 0:
                assert have == b"\t".join(row.split(b"\t")[:4]) + b"\t", (p, have[:40])
            else:
                assert have == b""


def test_one_file_of_60_samples():
    slab = make_slab(96, 60, seed=301, coverage=0.3, indel_frac=0.05)
    got, _ = compare(slab, [60])
    from basevar_amd import _capi
    assert got.n_variant > 0 and (got.row_state & _capi.BV_TEXT_INDEL).any()


def test_seven_files_of_200_and_one_of_37_with_groups():
    slab = make_slab(40, 7 * 200 + 37, seed=302, coverage=0.1, indel_frac=0.02, n_groups=2)
    compare(slab, [200] * 7 + [37], n_groups=2)
    slab["rpr"][5, :50] = np.where(slab["base_strand"][5, :50] != 8, 9000 + np.arange(50), 0)
    compare(slab, [200] * 7 + [37], n_groups=2, level=6)


def test_depth_zero_positions_give_no_record():
    from basevar_amd import _capi
    slab = make_slab(32, 400, seed=305, coverage=0.1)
    slab["base_strand"][[3, 17], :] = 8
    for k in ("qual", "mapq", "rpr"):
        slab[k][[3, 17], :] = 0
    got, _ = compare(slab, [200, 200], depth_zero=(9, 25))
    assert (got.row_state[[3, 9, 17, 25]] == _capi.BV_TEXT_SKIP).all()


def test_rows_of_ten_thousand_samples_span_many_members():
    slab = make_slab(24, 10000, seed=303, coverage=0.08)  # (the slab of test_gpu_text_rows.py: it has variant sites)
    text, row_off = slab_rows(slab, [10000])
    assert int(row_off[1]) > 0xff00  # one row is longer than a member holds
    got, _ = compare(slab, [10000])
    assert got.n_variant > 0


@pytest.mark.parametrize("member", [0x100, 0x1000, 0xff00])
def test_member_sizes_headers_and_a_last_line_without_newline(member):
    slab = make_slab(24, 10 * 200, seed=308, coverage=0.08, indel_frac=0.01)
    compare(slab, [200] * 10, member=member, headers=[3, 0, 1, 7, 2, 2, 0, 5, 1, 4], last_newline=False)


@pytest.mark.parametrize("window", [1, 7, 1000])
def test_windows_chained_through_the_cursors(window):
    """the same files taken `window` positions at a time, every run starting at the member the last cursor names: the
    concatenation is the one-call result"""
    from basevar_amd import _capi
    fs = [200, 120, 37]
    P, N, F = 30, sum(fs), len(fs)
    slab = make_slab(P, N, seed=309, coverage=0.1, indel_frac=0.02, n_groups=2)
    text, row_off = slab_rows(slab, fs)
    headers = [2, 0, 5]
    sizes = [0x1000, 0x100, 0xff00]
    files = [members_of(t, m) for t, m in zip(file_texts(text, row_off, P, F, headers), sizes)]
    eng = engine(P, N)
    try:
        exp = eng.lrt_text((text, row_off), fs, group_id=slab["group_id"], n_groups=2)
        at = [0] * F          # member of the file where the next run starts
        skip_b = [0] * F
        skip_l = list(headers)
        parts, done = [], 0
        while done < P:
            runs = [files[f][at[f]:] for f in range(F)]
            got = eng.lrt_bgzf(runs, fs, skip_bytes=skip_b, skip_lines=skip_l, max_positions=window, group_id=slab["group_id"], n_groups=2)
            n = got.row_state.shape[0]
            assert n == min(window, P - done)
            check_fetched(got, text, row_off, P, F, first=done)
            parts.append((got, done))
            done += n
            for f in range(F):
                at[f] += int(got.cursors[f, 0])
                skip_b[f] = int(got.cursors[f, 1])
            skip_l = [0] * F
        # nothing is left: no position, and the cursors stay where they are
        runs = [files[f][at[f]:] for f in range(F)]
        got = eng.lrt_bgzf(runs, fs, skip_bytes=skip_b, max_positions=window)
        assert got.row_state.shape[0] == 0 and len(got.sites) == 0
    finally:
        eng.close()
    assert np.array_equal(np.concatenate([g.row_state for g, _ in parts]), exp.row_state)
    assert np.array_equal(np.concatenate([g.positions + d for g, d in parts]), exp.positions)
    assert b"".join(g.sites.tobytes() for g, _ in parts) == exp.sites.tobytes()
    assert b"".join(g.groups.tobytes() for g, _ in parts) == exp.groups.tobytes()
    assert b"".join(g.cell.tobytes() for g, _ in parts) == exp.cell.tobytes()
    assert b"".join(g.phred.tobytes() for g, _ in parts) == exp.phred.tobytes()
    assert not (exp.row_state & _capi.BV_TEXT_HOST).any()


def test_rows_left_to_the_host_and_indel_rows():
    """CRLF, a ragged column, a covered call with strand '.', signed numbers: BV_TEXT_HOST, fetched whole, read by the host
    reader; the records are lrt_text's.  A capacity that is too small reports the size and writes nothing."""
    from basevar_amd import _capi
    fs = [100, 100]
    P, N, F = 12, 200, 2
    slab = make_slab(P, N, seed=307, coverage=0.2, indel_frac=0.03)
    text, off = slab_rows(slab, fs)
    rows = [[bytes(text[int(off[p * 2 + f]):int(off[p * 2 + f + 1]) - 1]) for f in range(2)] for p in range(P)]

    def sign_mapq(row):
        c = row.split(b"\t")
        c[4] = b" ".join(b"+" + t for t in c[4].split(b" "))
        return b"\t".join(c)

    def dot_strand(row):  # the first covered call gets strand '.'
        c = row.split(b"\t")
        bases, strands = c[5].split(b" "), c[8].split(b" ")
        k = next(i for i, b in enumerate(bases) if b in (b"A", b"C", b"G", b"T"))
        strands[k] = b"."
        c[8] = b" ".join(strands)
        return b"\t".join(c)
    rows[2] = [r + b"\r" for r in rows[2]]                       # CRLF
    rows[4] = [sign_mapq(r) for r in rows[4]]
    rows[6] = [rows[6][0], rows[6][1].rsplit(b" ", 1)[0]]        # a ragged column: one strand token short
    rows[7] = [b"\t".join(c[:3] + [b"+0"] + c[4:]) for c in (r.split(b"\t") for r in rows[7])]
    rows[9] = [dot_strand(rows[9][0]), rows[9][1]]
    flat_text = b"".join(r + b"\n" for pos in rows for r in pos)
    flat_off = np.concatenate([[0], np.cumsum([len(r) + 1 for pos in rows for r in pos])]).astype(np.uint64)

    def reader(lines):
        try:
            got = _py_host_reader(N)([l.rstrip(b"\r") for l in lines])
        except (ValueError, IndexError):
            return None  # (rows this simple reader cannot take are skipped, in both paths alike)
        return got if got is not None and all(len(a) == N for a in got[:4]) else None
    eng = engine(P, N)
    try:
        exp = eng.lrt_text(rows, fs, host_reader=reader)
        runs = [members_of(b"".join(rows[p][f] + b"\n" for p in range(P)), 0x400) for f in range(F)]
        got = eng.lrt_bgzf(runs, fs, host_reader=reader)
        need = int(got.fetched[0].size)
        guard = np.full(need + 64, 0xA5, np.uint8)
        roff = np.full(P * F + 1, 0x5A5A5A5A, np.uint64)
        import ctypes as C
        n = C.c_uint64(0)
        assert eng._lib.bv_engine_text_rows_fetch(eng._h, guard.ctypes.data, need - 1, roff.ctypes.data, C.byref(n), None) == 0
        assert n.value == need and (guard == 0xA5).all() and (roff == 0x5A5A5A5A).all()
        assert eng.text_rows_fetch(P * F, capacity=3) == (None, need)
        again, roff2 = eng.text_rows_fetch(P * F)
        assert again.tobytes() == got.fetched[0].tobytes() and np.array_equal(roff2, got.fetched[1])
    finally:
        eng.close()
    host = [2, 4, 6, 7, 9]
    assert (exp.row_state[host] & (_capi.BV_TEXT_HOST | _capi.BV_TEXT_SKIP)).all()
    assert (exp.row_state[[2, 4, 9]] == _capi.BV_TEXT_HOST).all()
    same_batch(got, exp, 0)
    assert (got.row_state & _capi.BV_TEXT_INDEL).any()
    check_fetched(got, np.frombuffer(flat_text, np.uint8), flat_off, P, F, host_positions=host)


def test_a_damaged_member_in_file_2_of_3():
    from basevar_amd import _capi
    fs = [50, 50, 50]
    P, N, F = 20, 150, 3
    slab = make_slab(P, N, seed=310, coverage=0.2)
    text, row_off = slab_rows(slab, fs)
    runs = [members_of(t, 0x800) for t in file_texts(text, row_off, P, F)]
    assert len(runs[2]) > 4
    good = runs[2][3]
    bad = bytearray(good)
    bad[-5] ^= 0x40  # the CRC32 field
    eng = engine(P, N)
    try:
        runs[2][3] = bytes(bad)
        with pytest.raises(RuntimeError, match=r"file 2, member 3 of its run: BGZF status 4") as ei:
            eng.lrt_bgzf(runs, fs)
        assert ei.value.args[1] == _capi.BV_ERR_DATA
        out = np.zeros(1, dtype=_capi.SITE_DTYPE)  # nothing was parsed: there is nothing to submit or to fetch
        assert eng._lib.bv_engine_text_submit(eng._h, None, None, 1, out.ctypes.data, None, None, None, None) == _capi.BV_ERR_INVALID_ARG
        with pytest.raises(RuntimeError, match="no bv_engine_text_parse_bgzf"):
            eng.text_rows_fetch(P * F)
        runs[2][3] = good
        got = eng.lrt_bgzf(runs, fs)
        exp = eng.lrt_text((text, row_off), fs)
    finally:
        eng.close()
    same_batch(got, exp, 0)


def test_argument_errors():
    from basevar_amd import _capi
    fs = [50]
    slab = make_slab(4, 50, seed=311, coverage=0.2)
    text, row_off = slab_rows(slab, fs)
    runs = [members_of(file_texts(text, row_off, 4, 1)[0], 0x800)]
    eng = engine(4, 50)
    try:
        for kw in (dict(skip_bytes=[1 << 30]), dict(max_positions=0), dict(file_samples=[0]), dict(file_samples=[51]), dict(n_groups=2)):
            args = dict(runs=runs, file_samples=fs)
            args.update(kw)
            with pytest.raises(RuntimeError, match=r"bv_engine_text_parse_bgzf failed \(-1\)"):
                eng.lrt_bgzf(**args)
        assert eng._lib.bv_engine_text_parse_bgzf(eng._h, None, None, 0, None, None, None, None) == _capi.BV_ERR_INVALID_ARG
        assert len(eng.lrt_bgzf(runs, fs).sites) > 0
    finally:
        eng.close()


# ---- members written by zlib and written again by tests/deflate_writer.py under codes zlib's compressor never chooses


def transcoded_members(data, member, level=1, cut=150, stored_every=5):
    """members_of(), every member's tokens written again: dynamic blocks of `cut` tokens under skewed codes of up to 15 bits over
    all 286 + 30 symbols (every other block with its data in the longest codes), HCLEN 19, every stored_every-th block stored; zlib inflates each to the same text"""
    import zlib
    import deflate_writer as dw
    out = []
    for at in range(0, len(data), member):
        part = data[at:at + member]
        payload, text = dw.transcode(bc.deflate(part, level), cut=cut, stored_every=stored_every)
        assert text == part and zlib.decompress(payload, -15) == part
        out.append(bc.wrap(payload, part))
        assert len(out[-1]) <= 65536
    return out + [bc.member(b"")]


def tokens_at_distance(before, text, dist):
    """text as tokens behind `before`: matches at exactly `dist` wherever at least three bytes repeat there, else literals"""
    assert len(before) >= dist
    whole, tokens, i = before + text, [], 0
    base = len(before)
    while i < len(text):
        n = 0
        while n < 258 and i + n < len(text) and whole[base + i + n] == whole[base + i + n - dist]:
            n += 1
        if n >= 3:
            tokens.append((n, dist))
            i += n
        else:
            tokens.append(text[i])
            i += 1
    return tokens


def test_rows_from_transcoded_members():
    import deflate_writer as dw
    slab = make_slab(40, 3 * 200 + 37, seed=312, coverage=0.1, indel_frac=0.02, n_groups=2)
    compare(slab, [200] * 3 + [37], n_groups=2, member=0x6000, members_of=transcoded_members)
    f = dw.trace(bc.payload_of(transcoded_members(bc.rows_text(0x6000, seed=9), 0x6000)[0])).features
    assert f["hclen19_slot18_nonzero"] and f["hlit:286"] and f["hdist:30"] and f["blocks:0"] and f["blocks:2"] > 5
    assert f["lit_bits:15"] and f["dist_bits:15"]


def repeated_block_file(P_tail=25, N=60, seed=313):
    """(rows [[bytes]] per position, members): one file whose first 2 * 32 768 bytes are a block of rows and the same rows again
    at the next positions (CHROM padded so that the block is 32 768 bytes), the second block written as matches at distance
    32 768 with literals where POS differs; everything under transcoded codes"""
    import zlib
    import deflate_writer as dw
    slab = make_slab(200, N, seed=seed, coverage=0.3, indel_frac=0.02)
    text, off = slab_rows(slab, [N])
    P_block = int(np.searchsorted(off, 32768, side="right")) - 1  # the rows that fit 32 768 bytes
    assert 20 < P_block and 2 * P_block + P_tail <= 200
    slab["base_strand"][P_block:2 * P_block] = slab["base_strand"][:P_block]
    for k in ("qual", "mapq", "rpr", "ref_base"):
        slab[k][P_block:2 * P_block] = slab[k][:P_block]
    text, off = slab_rows(slab, [N])
    rows = [bytes(text[int(off[p]):int(off[p + 1]) - 1]) for p in range(2 * P_block + P_tail)]
    short = 32768 - sum(len(r) + 1 for r in rows[:P_block])
    assert 0 <= short < 25 * P_block, short
    for p in range(2 * P_block):  # a longer CHROM: short // P_block letters, one more on the first short % P_block rows
        j = p % P_block
        rows[p] = b"chr9" + b"x" * (short // P_block + (j < short % P_block)) + rows[p][4:]
    first, second = (b"".join(r + b"\n" for r in rows[a:a + P_block]) for a in (0, P_block))
    assert len(first) == len(second) == 32768 and first != second
    extra = tokens_at_distance(first, second, 32768)
    payload, both = dw.transcode(bc.deflate(first, 6), cut=400, stored_every=7, extra_tokens=extra)
    assert both == first + second and zlib.decompress(payload, -15) == both
    f = dw.trace(payload).features
    assert f["dist_32768"] > 100 and f["dist_32768"] > len(extra) // 2 and f["hclen19_slot18_nonzero"]
    head = bc.wrap(payload, both)
    assert len(head) <= 65536
    tail = b"".join(r + b"\n" for r in rows[2 * P_block:])
    return rows, [head] + transcoded_members(tail, 0x3000, 6)


def test_rows_repeated_at_distance_32768():
    from basevar_amd import _capi
    N = 60
    rows, members = repeated_block_file(N=N)
    P = len(rows)
    flat = np.frombuffer(b"".join(r + b"\n" for r in rows), np.uint8)
    row_off = np.concatenate([[0], np.cumsum([len(r) + 1 for r in rows])]).astype(np.uint64)
    eng = engine(P, N)
    try:
        exp = eng.lrt_text([[r] for r in rows], [N])
        got = eng.lrt_bgzf([members], [N])
    finally:
        eng.close()
    assert got.row_state.shape == (P, 1) and not (got.row_state & _capi.BV_TEXT_HOST).any()
    same_batch(got, exp, 0)
    assert got.n_variant > 0
    check_fetched(got, flat, row_off, P, 1)


# ---- the positional corpus of the row parser (tests/cpp/row_lane_cases.hpp) through the line index
def tolerant_reader(N, seen=None):
    """_py_host_reader for rows it may not be able to take: those are skipped (in both paths alike); `seen` collects the lines of
    every position it was asked for"""
    def reader(lines):
        if seen is not None:
            seen.add(tuple(lines))
        try:
            got = _py_host_reader(N)([l.rstrip(b"\r") for l in lines])
        except (ValueError, IndexError, OverflowError):
            return None
        return got if got is not None and all(len(a) == N for a in got[:4]) else None
    return reader


def lane_corpus(tmp_path):
    """{samples per file: [(valid, kind, [row per file])]}: the cases of the corpus that can stand in a file of lines and that the
    C++ host reader does not throw on (text_rows_check <n> lanes-dump)"""
    import subprocess
    from test_gpu_text_rows import build_text_rows_check
    path = tmp_path / "lane_cases.txt"
    subprocess.check_call([build_text_rows_check(tmp_path), "0", "lanes-dump", str(path)], stdout=subprocess.DEVNULL)
    lines = open(path, "rb").read().split(b"\n")
    groups, i = {}, 0
    while i < len(lines) and lines[i].startswith(b"CASE "):
        _, valid, fs, kind = lines[i].split(b" ", 3)
        fs = tuple(int(x) for x in fs.split(b","))
        groups.setdefault(fs, []).append((valid == b"1", kind.decode("latin-1"), lines[i + 1:i + 1 + len(fs)]))
        i += 1 + len(fs)
    assert i == len(lines) - 1 and lines[-1] == b""
    return groups


def test_positional_corpus_through_the_line_index(tmp_path):
    """the valid sweep and the damaged rows the host reader does not throw on, written as BGZF files: the kernel gets row_beg /
    row_end from the line index instead of contiguous offsets, the host reader gets rows fetched from the device; row_state and
    records are lrt_text's on the same rows uncompressed"""
    from basevar_amd import _capi
    groups = lane_corpus(tmp_path)
    assert sum(len(c) for c in groups.values()) > 250 and len(groups) >= 2
    for fs, cases in groups.items():
        P, N, F = len(cases), sum(fs), len(fs)
        rows = [c[2] for c in cases]
        valid = np.array([c[0] for c in cases])
        flat = b"".join(r + b"\n" for pos in rows for r in pos)
        flat_off = np.concatenate([[0], np.cumsum([len(r) + 1 for pos in rows for r in pos])]).astype(np.uint64)
        seen = set()
        eng = engine(P, N)
        try:
            exp = eng.lrt_text(rows, list(fs), host_reader=tolerant_reader(N, seen))
            runs = [members_of(b"".join(rows[p][f] + b"\n" for p in range(P)), 0x1300) for f in range(F)]
            got = eng.lrt_bgzf(runs, list(fs), host_reader=tolerant_reader(N))
        finally:
            eng.close()
        assert got.row_state.shape == (P, F)
        assert not (exp.row_state[valid] & (_capi.BV_TEXT_HOST | _capi.BV_TEXT_SKIP)).any(), "a row of the valid sweep was not parsed on the device"
        same_batch(got, exp, 0)
        host = [p for p in range(P) if tuple(rows[p]) in seen]
        if len(fs) == 3:
            on_device = ((exp.row_state[:, 0] & (_capi.BV_TEXT_HOST | _capi.BV_TEXT_SKIP)) == 0).sum()
            assert len(host) > 50 and on_device >= valid.sum() > 100 and (exp.row_state & _capi.BV_TEXT_INDEL).any()
        check_fetched(got, np.frombuffer(flat, np.uint8), flat_off, P, F, host_positions=host)


# ---- the line index at the edges of its 16 KiB tiles (bv_text_line_count / _scan / _scatter_kernel): rows built as bytes, an
# insertion token in sample 0 pads a row to an exact length (such a row is parsed on the device and fetched whole)
TILE = 16384


def pad_row(pos, n, salt, length=None):
    """one row of n samples with its line break; with `length`, exactly that many bytes (None if that is too short)"""
    cols = [[], [], [], [], []]
    cov = 0
    for i in range(n):
        k = (i * 7 + salt * 3 + pos) % 11
        if length is not None and i == 0:
            tok = (b"60", b"+A", b"I", b"9", b"+")
        elif k < 4:
            tok = (b"%d" % (20 + (i * 13 + salt) % 41), b"ACGT"[k:k + 1], bytes([38 + (i * 5 + salt) % 36]), b"%d" % (1 + (i * 11 + salt) % 150),
                   b"-" if (i + salt) % 2 else b"+")
        else:
            tok = (b"0", b"N", b"!", b"0", b".")
        cov += tok[1] != b"N"
        for c in range(5):
            cols[c].append(tok[c])
    if cov == 0:
        cols[0][-1], cols[1][-1], cols[2][-1], cols[3][-1], cols[4][-1] = b"33", b"C", b"F", b"12", b"-"
        cov = 1
    row = b"chr7\t%d\tA\t%d\t" % (pos, cov) + b"\t".join(b" ".join(c) for c in cols) + b"\n"
    if length is None:
        return row
    if length < len(row):
        return None
    cols[1][0] = b"+A" + b"C" * (length - len(row))
    return b"chr7\t%d\tA\t%d\t" % (pos, cov) + b"\t".join(b" ".join(c) for c in cols) + b"\n"


def plain_rows(n_rows, n, salt, first=1):
    return [pad_row(first + p, n, salt) for p in range(n_rows)]


def fit_newline(rows, n, salt, at, first=1):
    """the rows with one of them padded so that its line break is byte `at` of their concatenation; (rows, its index)"""
    ends = np.cumsum([len(r) for r in rows])  # ends[j] - 1: row j's line break
    j = int(np.searchsorted(ends - 1, at, side="right")) - 1
    while j >= 0:
        row = pad_row(first + j, n, salt, len(rows[j]) + at - int(ends[j] - 1))
        if row is not None:
            out = rows[:j] + [row] + rows[j + 1:]
            assert b"".join(out)[at:at + 1] == b"\n" and b"".join(out[:j + 1]).endswith(b"\n") and len(b"".join(out[:j + 1])) == at + 1
            return out, j
        j -= 1
    raise AssertionError("no row in front of byte %d" % at)


def lines_behind(text, skip_b, skip_l, at_end):
    """(begin, end, offset of the first byte behind) of every line the index must take from a run: the complete lines behind
    skip_b bytes and skip_l further lines, and with at_end an unterminated last one"""
    out, at = [], skip_b
    while True:
        nl = text.find(b"\n", at)
        if nl < 0:
            if at_end and at < len(text):
                out.append((at, len(text), len(text)))
            break
        out.append((at, nl, nl + 1))
        at = nl + 1
    return out[skip_l:]


def cursor_of(members_text, x):
    """(member, offset) of inflated byte x of a run whose members hold members_text bytes each: the first member that reaches
    beyond x; (number of members, 0) behind the last"""
    k = base = 0
    while k < len(members_text) and base + members_text[k] <= x:
        base += members_text[k]
        k += 1
    return [k, x - base if k < len(members_text) else 0]


def index_check(eng, texts, fs, skip_bytes=None, skip_lines=None, at_end=True, max_positions=None, member=0x5000, want_positions=None):
    """lrt_bgzf on the files' texts against what their bytes say: the number of positions, the cursors, the fetched text and --
    through lrt_text on the same rows uncompressed -- row_state and records.  Returns (got, expected first bytes not taken)."""
    F = len(fs)
    sb = list(skip_bytes) if skip_bytes is not None else [0] * F
    sl = list(skip_lines) if skip_lines is not None else [0] * F
    lines = [lines_behind(texts[f], sb[f], sl[f], at_end) for f in range(F)]
    P = min([len(l) for l in lines] + [eng.max_sites] + ([max_positions] if max_positions is not None else []))
    if want_positions is not None:
        assert P == want_positions, (P, want_positions)
    rows = [[texts[f][lines[f][p][0]:lines[f][p][1]] for f in range(F)] for p in range(P)]
    x = [lines[f][P - 1][2] if P else sb[f] for f in range(F)]
    sizes = [[min(member, len(t) - at) for at in range(0, len(t), member)] + [0] for t in texts]
    got = eng.lrt_bgzf([members_of(t, member) for t in texts], fs, skip_bytes=sb, skip_lines=sl, at_end=at_end, max_positions=max_positions)
    assert got.row_state.shape == (P, F), (got.row_state.shape, P)
    assert got.cursors.tolist() == [cursor_of(sizes[f], x[f]) for f in range(F)], (got.cursors.tolist(), x)
    if P:
        exp = eng.lrt_text(rows, fs)  # (raises if a position is not in the strict form)
        same_batch(got, exp, 0)
        flat = np.frombuffer(b"".join(r + b"\n" for pos in rows for r in pos), np.uint8)
        off = np.concatenate([[0], np.cumsum([len(r) + 1 for pos in rows for r in pos])]).astype(np.uint64)
        check_fetched(got, flat, off, P, F)
    else:
        assert len(got.sites) == 0 and got.fetched[0].size == 0
    return got, x


FS3 = [36, 40, 44]  # rows of about 400, 440 and 480 bytes: 90 rows are three tiles in every file
HEAD = [b"#" + b"h" * 35 + b"\n", b"#" + b"h" * 19 + b"\n", b"#" + b"h" * 51 + b"\n"]  # 37, 21 and 53 bytes: no multiple of 16


@pytest.mark.parametrize("headers", [False, True])
def test_line_breaks_on_the_last_and_first_byte_of_a_tile(headers):
    """a row's line break on bytes 16383, 16384, 32767 and 32768 behind skip_bytes, in file 0 and in the last file"""
    from basevar_amd import _capi
    P, F = 90, 3
    skip = [len(h) if headers else 0 for h in HEAD]
    eng = engine(128, sum(FS3))
    try:
        for at in (TILE - 1, TILE, 2 * TILE - 1, 2 * TILE):
            texts, hit = [], []
            for f in range(F):
                rows = plain_rows(P, FS3[f], f)
                if f != 1:
                    rows, j = fit_newline(rows, FS3[f], f, at)
                    hit.append(j)
                texts.append((HEAD[f] if headers else b"") + b"".join(rows))
                if f != 1:
                    assert texts[f][skip[f] + at] == 10 and 2 * TILE < len(texts[f]) - skip[f] <= 4 * TILE
            got, _ = index_check(eng, texts, FS3, skip_bytes=skip, want_positions=P)
            assert (got.row_state[hit[0], 0] & _capi.BV_TEXT_INDEL) and (got.row_state[hit[1], 2] & _capi.BV_TEXT_INDEL)
    finally:
        eng.close()


def test_a_line_break_on_every_lane_of_the_scatter_kernel():
    """the scatter kernel finds line ends with 64-byte ballots: rows of 64 consecutive pad lengths, twice, so that -- read back
    from the built bytes -- a line break falls on each of the 64 lanes, behind a skip that is no multiple of 64"""
    P, n = 128, 40
    rows = [pad_row(1 + p, n, 0, 450 + p % 64) for p in range(P)]
    text0 = HEAD[0] + b"".join(rows)
    lanes = {(i - len(HEAD[0])) % 64 for i in range(len(HEAD[0]), len(text0)) if text0[i] == 10}
    assert lanes == set(range(64))
    assert {len(r) for r in rows} == set(range(450, 514))
    eng = engine(P, n + 20)
    try:
        index_check(eng, [text0, b"".join(plain_rows(P, 20, 1))], [n, 20], skip_bytes=[len(HEAD[0]), 0], want_positions=P)
    finally:
        eng.close()


@pytest.mark.parametrize("size", [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1])
def test_runs_that_end_on_a_tile_boundary(size):
    """file 0's bytes behind its skip are exactly `size`: with the last line terminated; unterminated at the end of the file (the
    spare line break then lies at byte `size`, for 16384 and 32768 in a tile of its own -- the row is counted, parsed and fetched);
    unterminated with at_end = 0 (the partial line is no position and the cursor points at its first byte)"""
    n, m = 40, 24
    eng = engine(128, n + m)
    try:
        for skip0 in (0, len(HEAD[0])):
            head = HEAD[0] if skip0 else b""
            rows, j = fit_newline(plain_rows(100, n, 0), n, 0, size - 1)
            whole = head + b"".join(rows[:j + 1])                       # terminated: `size` bytes behind the skip
            rows_u, ju = fit_newline(plain_rows(100, n, 0), n, 0, size)
            cut = head + b"".join(rows_u[:ju + 1])[:-1]                 # unterminated: `size` bytes, the line break would be byte `size`
            assert len(whole) - skip0 == size and len(cut) - skip0 == size and whole.endswith(b"\n") and not cut.endswith(b"\n")
            other = b"".join(plain_rows(max(j, ju) + 6, m, 1))
            for at_end in (True, False):
                index_check(eng, [whole, other], [n, m], skip_bytes=[skip0, 0], at_end=at_end, want_positions=j + 1)
            got, x = index_check(eng, [cut, other], [n, m], skip_bytes=[skip0, 0], at_end=True, want_positions=ju + 1)
            assert x[0] == len(cut)
            got, x = index_check(eng, [cut, other], [n, m], skip_bytes=[skip0, 0], at_end=False, want_positions=ju)
            assert x[0] == len(head) + len(b"".join(rows_u[:ju])) and cut[x[0] - 1:x[0]] == b"\n"
            # ... and the same in the last file
            index_check(eng, [other, cut], [m, n], skip_bytes=[0, skip0], at_end=True, want_positions=ju + 1)
            index_check(eng, [other, cut], [m, n], skip_bytes=[0, skip0], at_end=False, want_positions=ju)
    finally:
        eng.close()


def test_more_header_lines_than_the_first_tile_holds():
    """skip_lines beyond the lines of the first tile: 700 header lines, more than 16 KiB of them"""
    heads = [b"".join(b"##header of file %d line %d\n" % (f, k) for k in range(nk)) for f, nk in ((0, 700), (1, 3), (2, 0))]
    assert len(heads[0]) > TILE + 1000 and heads[0][:TILE].count(b"\n") < 700
    texts = [heads[f] + b"".join(plain_rows(60, FS3[f], f)) for f in range(3)]
    eng = engine(64, sum(FS3))
    try:
        index_check(eng, texts, FS3, skip_lines=[700, 3, 0], want_positions=60)
        index_check(eng, texts, FS3, skip_lines=[700, 3, 0], want_positions=59, at_end=False, skip_bytes=None, max_positions=59)
        index_check(eng, [t[:-1] for t in texts], FS3, skip_lines=[700, 3, 0], want_positions=59, at_end=False)
    finally:
        eng.close()


def test_one_tile_beside_three():
    """files of very different length: the minimum over the files decides, the long files' cursors stop inside their runs"""
    texts = [b"".join(plain_rows(110, FS3[0], 0)), b"".join(plain_rows(30, FS3[1], 1)), b"".join(plain_rows(95, FS3[2], 2))]
    assert len(texts[1]) < TILE and 2 * TILE < len(texts[0]) <= 3 * TILE and 2 * TILE < len(texts[2]) <= 3 * TILE
    eng = engine(128, sum(FS3))
    try:
        got, x = index_check(eng, texts, FS3, want_positions=30)
        assert x[1] == len(texts[1]) and x[0] < TILE and x[2] < TILE
        index_check(eng, [texts[1], texts[0], texts[2]], [FS3[1], FS3[0], FS3[2]], want_positions=30)
        index_check(eng, [texts[0], texts[2], texts[1][:-1]], [FS3[0], FS3[2], FS3[1]], want_positions=29, at_end=False)
    finally:
        eng.close()


@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_file_with_nothing_behind_its_skip(where):
    """len == skip_bytes in one file (first, in the middle, last) beside files that have text: no position, no error, and the
    cursors stay where they started"""
    eng = engine(64, sum(FS3))
    try:
        for empty, skip in ((HEAD[0], len(HEAD[0])), (b"", 0)):
            texts = [HEAD[f] + b"".join(plain_rows(50, FS3[f], f)) for f in range(3)]
            sb = [len(h) for h in HEAD]
            texts[where], sb[where] = empty, skip
            for at_end in (True, False):
                got, x = index_check(eng, texts, FS3, skip_bytes=sb, at_end=at_end, want_positions=0)
                assert x == sb
        texts[where] = HEAD[where] + b"".join(plain_rows(50, FS3[where], where))  # ... and the engine goes on
        index_check(eng, texts, FS3, skip_bytes=[len(h) for h in HEAD], want_positions=50)
    finally:
        eng.close()


@pytest.mark.parametrize("at", [TILE - 1, TILE])
def test_max_positions_cuts_at_a_tile_boundary(at):
    """max_positions ends the window with a row whose line break is the last byte of a tile (16383) or the first byte of the next
    (16384), in file 0 and in the last file; the next window, started from the cursors, goes on exactly there and the two
    together are the one-call result"""
    P, F, member = 90, 3, 0x2800
    texts, hit = [], []
    for f in range(F):
        rows = plain_rows(P, FS3[f], f)
        if f != 1:
            rows, j = fit_newline(rows, FS3[f], f, at)
            hit.append(j)
        texts.append(b"".join(rows))
    eng = engine(128, sum(FS3))
    try:
        whole, _ = index_check(eng, texts, FS3, member=member, want_positions=P)
        for cut in sorted({hit[0] + 1, hit[1] + 1}):
            first, x = index_check(eng, texts, FS3, member=member, max_positions=cut, want_positions=cut)
            assert all(texts[f][x[f] - 1] == 10 for f in range(F)) and (x[0] == at + 1 or x[2] == at + 1)
            # the next window: from the member each cursor names, skip_bytes = its offset
            files = [members_of(t, member) for t in texts]
            runs = [files[f][int(first.cursors[f, 0]):] for f in range(F)]
            rest = eng.lrt_bgzf(runs, FS3, skip_bytes=[int(c) for c in first.cursors[:, 1]])
            assert rest.row_state.shape[0] == P - cut
            assert np.array_equal(np.concatenate([first.row_state, rest.row_state]), whole.row_state)
            assert np.array_equal(np.concatenate([first.positions, rest.positions + cut]), whole.positions)
            assert first.sites.tobytes() + rest.sites.tobytes() == whole.sites.tobytes()
            assert first.cell.tobytes() + rest.cell.tobytes() == whole.cell.tobytes() and first.phred.tobytes() + rest.phred.tobytes() == whole.phred.tobytes()
            tail = [t[x[f]:] for f, t in enumerate(texts)]
            rows = [[l for l in tail[f].split(b"\n")[:-1]] for f in range(F)]
            flat = np.frombuffer(b"".join(rows[f][p] + b"\n" for p in range(P - cut) for f in range(F)), np.uint8)
            off = np.concatenate([[0], np.cumsum([len(rows[f][p]) + 1 for p in range(P - cut) for f in range(F)])]).astype(np.uint64)
            check_fetched(rest, flat, off, P - cut, F)
    finally:
        eng.close()
