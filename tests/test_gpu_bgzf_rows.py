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
