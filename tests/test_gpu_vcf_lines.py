"""GPU tests of bv_engine_vcf_format / _fetch / _deflate (include/basevar_amd_vcf.h): the lines the device writes are, byte for
byte, the lines host/vcf_emit.hpp's format_vcf_line writes for the same planes, heads and records -- printed by the stand-alone
harness tests/cpp/vcf_lines_check.cpp -- at every size, coverage and alignment at which the kernels of
basevar_amd/csrc/bv_vcf.hip take another path; nothing outside the text is touched; the members are bgzf_deflate's."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vcf_lines_ref as vr  # noqa: E402

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def harness():
    return vr.build()


@pytest.fixture(scope="module")
def T():
    from basevar_amd import _capi
    return int(_capi.load().bv_vcf_tile_samples())


def engine(P, N):
    import basevar_amd as bv
    return bv.BaseTypeEngine(max_sites=max(P, 1), min_af_value=bv.min_af(max(N, 1)), device=0, max_samples=max(N, 1))


def planes(rng, covered):
    """cell / phred rows for a boolean coverage matrix: covered cells 0-7, the others BV_CELL_N / _INS / _DEL; any phred"""
    cell = np.where(covered, rng.integers(0, 8, covered.shape), rng.choice([8, 9, 10], covered.shape)).astype(np.uint8)
    return cell, rng.integers(0, 256, covered.shape).astype(np.uint8)


def coverage_rows(rng, n, T):
    """none, all, alternating, only the first / the last sample of each 64-sample step and of each tile, random at 0.08"""
    s = np.arange(n)
    last_of_tile = (s % T == T - 1) | (s == n - 1)
    last_of_step = (s % 64 == 63) | (s == n - 1)
    return np.stack([np.zeros(n, bool), np.ones(n, bool), s % 2 == 0, s % 64 == 0, last_of_step, s % T == 0, last_of_tile, rng.random(n) < 0.08])


class Padded:
    """rows [n_rows][n] inside planes of `pitch` bytes a row (16-byte aligned), the padding filled by `fill(shape)`; host
    arrays, and the same on the device on request"""

    def __init__(self, cell, phred, pitch=None, fill=None):
        n_rows, n = cell.shape
        self.n_rows, self.n = n_rows, n
        self.pitch = pitch or (n + 15) // 16 * 16
        assert self.pitch % 16 == 0 and self.pitch >= n
        self.host = []
        for a in (cell, phred):
            raw = np.zeros(n_rows * self.pitch + 16, np.uint8)
            at = (-raw.ctypes.data) % 16
            p = raw[at:at + n_rows * self.pitch].reshape(n_rows, self.pitch)
            p[:] = 8 if fill is None else fill(p.shape)
            p[:, :n] = a
            self.host.append((raw, p))
        self.dev = None

    def slab(self, device):
        from basevar_amd import _capi
        if device:
            import torch
            if self.dev is None:
                self.dev = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for _, p in self.host]
                torch.cuda.synchronize()
            ptrs = [int(t.data_ptr()) for t in self.dev]
        else:
            ptrs = [p.ctypes.data for _, p in self.host]
        return _capi.Slab(self.n_rows, self.n, self.pitch, ptrs[0], ptrs[1], None, None, None, None, 0,
                          _capi.BV_MEM_DEVICE if device else _capi.BV_MEM_HOST, 0, 0)


def choose_head_lens(cell, sites, T):
    """Head lengths for the lines over rows `sites`: every length 1 .. 40 among the first 40, each chosen (greedily, from
    the line lengths the formula gives) so that the lines and the tiles come to begin at every offset modulo 16."""
    n = cell.shape[1]
    left, out, at, line_res, tile_res = set(range(1, 41)), [], 0, set(), set()
    for k, s in enumerate(sites):
        c = cell[s]
        line_res.add(at % 16)
        before = [4 * t0 + 13 * int(((c[:t0] & 8) == 0).sum()) for t0 in range(0, n, T)]
        body = 4 * n + 13 * int(((c & 8) == 0).sum()) + 1

        def gain(hl):
            new_tiles = {(at + hl + b) % 16 for b in before} - tile_res
            return len(new_tiles) + (k + 1 < len(sites) and (at + hl + body) % 16 not in line_res)
        hl = max(sorted(left) if left else range(1, 41), key=gain)
        left.discard(hl)
        tile_res |= {(at + hl + b) % 16 for b in before}
        out.append(hl)
        at += hl + body
    assert not left
    return out


def make_lines(rng, sites, head_lens=None):
    """one seeded record per line; heads of the given lengths stand in the records' own heads' place"""
    lines = []
    for k, s in enumerate(sites):
        ref = int(rng.integers(0, 5))
        alts = [int(a) for a in rng.permutation(4)[:int(rng.integers(1, 4))]]
        head = None if head_lens is None else bytes(rng.integers(0x21, 0x7f, head_lens[k]).astype(np.uint8))
        lines.append(vr.line(s, vr.record(rng, alts)[0], ref_base=b"ACGTN"[ref:ref + 1], ref_pos=100 + k, head=head))
    return lines


def expected(harness, tmp_path, cell, phred, lines, names=()):
    exp = vr.run(harness, cell, phred, lines, names, tmp_dir=tmp_path)
    heads = [h for h, _, _ in exp]
    gt = np.stack([g for _, g, _ in exp])
    text = b"".join(t for _, _, t in exp)
    off = np.zeros(len(exp) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for _, _, t in exp])
    return heads, gt, text, off


def format_and_fetch(eng, sites, heads, gt, slab):
    off = eng.vcf_format(sites, heads, gt, slab)
    return off, eng.vcf_fetch().tobytes()


def test_every_cell_value_and_phred(harness, tmp_path):
    """one line of 11 x 256 samples holds every (cell, phred) pair the planes can hold"""
    rng = np.random.default_rng(21)
    cell = np.repeat(np.array(vr.CELL_VALUES, np.uint8), 256)[None, :]
    phred = np.tile(np.arange(256, dtype=np.uint8), len(vr.CELL_VALUES))[None, :]
    lines = [vr.line(0, vr.record(rng, [2, 0, 3])[0], ref_base=b"C")]
    heads, gt, text, off = expected(harness, tmp_path, cell, phred, lines)
    assert bytes(gt[0]) == b"2013"  # REF C; ALT G, A, T in that order
    P = Padded(cell, phred)
    eng = engine(1, cell.shape[1])
    try:
        got_off, got = format_and_fetch(eng, [0], heads, gt, P.slab(device=True))
    finally:
        eng.close()
    assert np.array_equal(got_off, off) and got == text


@pytest.mark.parametrize("n_case", range(9))
def test_sizes_coverages_and_alignments(harness, tmp_path, T, n_case):
    """n_samples around the 64-sample step and the tile; every coverage pattern; head lengths 1 .. 40 within one call; the
    lines and the tiles begin at every offset modulo 16 (asserted on the expected text alone)"""
    n = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1][n_case]
    rng = np.random.default_rng(100 + n_case)
    cov = coverage_rows(rng, n, T)
    cell, phred = planes(rng, cov)
    n_lines = 64
    sites = [k % cov.shape[0] for k in range(n_lines)]
    head_lens = choose_head_lens(cell, sites, T)
    assert set(head_lens[:40]) == set(range(1, 41))
    lines = make_lines(rng, sites, head_lens)
    heads, gt, text, off = expected(harness, tmp_path, cell, phred, lines)
    assert [len(h) for h in heads] == head_lens
    # where lines and tiles begin, from the expected lines alone: all 16 residues
    line_res, tile_res = set(), set()
    for k in range(n_lines):
        line_res.add(int(off[k]) % 16)
        c = cell[sites[k]]
        for t0 in range(0, n, T):
            tile_res.add((int(off[k]) + head_lens[k] + 4 * t0 + 13 * int(((c[:t0] & 8) == 0).sum())) % 16)
    assert line_res == set(range(16)) and tile_res == set(range(16)), (sorted(line_res), sorted(tile_res))
    P = Padded(cell, phred)
    eng = engine(cov.shape[0], n)
    try:
        got_off, got = format_and_fetch(eng, sites, heads, gt, P.slab(device=True))
    finally:
        eng.close()
    assert np.array_equal(got_off, off)
    if got != text:
        bad = next(i for i in range(min(len(got), len(text))) if got[i] != text[i])
        k = int(np.searchsorted(off, bad, side="right")) - 1
        raise AssertionError("first difference at byte %d: line %d (site %d, head %d bytes), byte %d of it" % (bad, k, sites[k], head_lens[k], bad - int(off[k])))


def test_padding_site_orders_and_untouched_neighbours(harness, tmp_path, T):
    """pitch > n_samples with random bytes (covered-looking cells among them) in the padding; site reversed, repeated and a
    strict subset; the bytes before and behind the text in a device buffer stay as they were"""
    import torch
    rng = np.random.default_rng(31)
    n = T + 37
    cov = np.concatenate([coverage_rows(rng, n, T), rng.random((8, n)) < 0.3])
    cell, phred = planes(rng, cov)
    R = cov.shape[0]
    P = Padded(cell, phred, pitch=(n + 15) // 16 * 16 + 48, fill=lambda shape: rng.integers(0, 256, shape).astype(np.uint8))
    eng = engine(R, n)
    try:
        for what, sites in (("reversed", list(range(R))[::-1]), ("repeated", [3, 3, 7, 3, 0, 0, R - 1, R - 1]), ("subset", [1, 4, 9, 14])):
            lines = make_lines(rng, sites, [5 + (3 * k) % 11 for k in range(len(sites))])
            heads, gt, text, off = expected(harness, tmp_path, cell, phred, lines)
            for device in (True, False):
                got_off = eng.vcf_format(sites, heads, gt, P.slab(device))
                assert np.array_equal(got_off, off), (what, device)
                total = int(off[-1])
                buf = torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                eng.vcf_fetch(dst_ptr=int(buf.data_ptr()) + 29, dst_capacity=total)
                got = buf.cpu().numpy()
                assert (got[:29] == SENTINEL).all() and (got[29 + total:] == SENTINEL).all(), (what, device)
                assert got[29:29 + total].tobytes() == text, (what, device)       # fetch to the device ...
                assert eng.vcf_fetch().tobytes() == text, (what, device)          # ... and to the host, host and device slab
    finally:
        eng.close()


def test_no_lines_and_a_second_call_replaces_the_text(harness, tmp_path):
    rng = np.random.default_rng(32)
    cell, phred = planes(rng, rng.random((3, 70)) < 0.5)
    P = Padded(cell, phred)
    eng = engine(3, 70)
    try:
        lines = make_lines(rng, [0, 1, 2], [4, 1, 9])
        heads, gt, text, off = expected(harness, tmp_path, cell, phred, lines)
        assert format_and_fetch(eng, [0, 1, 2], heads, gt, P.slab(True))[1] == text
        off0 = eng.vcf_format([], [], np.zeros((0, 4), np.uint8), P.slab(True))
        assert off0.tolist() == [0] and eng.vcf_fetch().size == 0
        members, moff = eng.vcf_deflate()
        assert members.size == 0 and moff.tolist() == [0]
        assert format_and_fetch(eng, [2], heads[2:], gt[2:], P.slab(False))[1] == text[int(off[2]):]
    finally:
        eng.close()


@pytest.mark.parametrize("level", ["fast", "small"])
def test_members_are_bgzf_deflates_of_the_fetched_text(harness, tmp_path, T, level):
    """vcf_deflate == bgzf_deflate(fetched text, the same cuts, the same level), byte for byte; zlib inflates the members to
    the text.  Cuts of 1, 64, 65 and 4,099 bytes, then of 0xff00."""
    rng = np.random.default_rng(41)
    n = 2 * T + 1
    cov = coverage_rows(rng, n, T)
    cell, phred = planes(rng, cov)
    sites = [k % 8 for k in range(24)]
    lines = make_lines(rng, sites)
    heads, gt, text, off = expected(harness, tmp_path, cell, phred, lines)
    total = len(text)
    assert total > 3 * 0xff00
    cuts = [0]
    for size in [1] * 5 + [64, 65, 4099, 1, 65, 64]:
        cuts.append(cuts[-1] + size)
    while cuts[-1] < total:
        cuts.append(min(total, cuts[-1] + 0xff00))
    cuts = np.array(cuts, np.uint64)
    eng = engine(8, n)
    try:
        got_off, got = format_and_fetch(eng, sites, heads, gt, Padded(cell, phred).slab(True))
        assert got == text
        for block_off in (cuts, None):
            members, moff = eng.vcf_deflate(block_off=block_off, level=level)
            ref_members, ref_moff = eng.bgzf_deflate(got, block_off=block_off, level=level)
            assert np.array_equal(moff, ref_moff) and members.tobytes() == ref_members.tobytes()
            back = b"".join(zlib.decompress(members[int(moff[k]):int(moff[k + 1])].tobytes(), 31) for k in range(len(moff) - 1))
            assert back == text
    finally:
        eng.close()


def test_refusals(harness, tmp_path):
    """every refusal of include/basevar_amd_vcf.h: BV_ERR_INVALID_ARG, a message, line_off / dst unwritten.  All of them are
    argument checks on the host: nothing is launched."""
    from basevar_amd import _capi
    rng = np.random.default_rng(51)
    n, R = 100, 4
    cell, phred = planes(rng, rng.random((R, n)) < 0.2)
    P = Padded(cell, phred)
    eng = engine(R, n)
    bad = _capi.BV_ERR_INVALID_ARG
    try:
        lib, h = eng._lib, eng._h
        site = np.array([0, 3, 1], np.uint32)
        head = np.frombuffer(b"abcdefghi", np.uint8).copy()
        head_off = np.array([0, 2, 5, 9], np.uint64)
        gt = np.frombuffer(b"0.1.01.22.0.", np.uint8).copy()
        line_off = np.full(4, 0x5a5a5a5a5a5a5a5a, np.uint64)
        dst = np.full(4096, SENTINEL, np.uint8)

        def fmt(slab=P.slab(False), site=site, head=head, head_off=head_off, gt=gt, n_lines=3, reserved=0, lines=True, out=line_off):
            ptr = lambda a: None if a is None else a.ctypes.data
            L = _capi.VcfLines(C.pointer(slab) if slab is not None else None, ptr(site), ptr(head), ptr(head_off), ptr(gt), n_lines, reserved)
            return lib.bv_engine_vcf_format(h, C.byref(L) if lines else None, ptr(out), None)

        def refused(rc, word):
            assert rc == bad and word in eng._err(), (rc, eng._err())
            assert (line_off == 0x5a5a5a5a5a5a5a5a).all() and (dst == SENTINEL).all()

        # before any format
        refused(lib.bv_engine_vcf_fetch(h, dst.ctypes.data, dst.size, _capi.BV_MEM_HOST, None), "no bv_engine_vcf_format")
        moff = np.zeros(2, np.uint64)
        boff = np.array([0, 10], np.uint64)
        refused(lib.bv_engine_vcf_deflate(h, boff.ctypes.data, 1, 0, dst.ctypes.data, dst.size, moff.ctypes.data, None), "no bv_engine_vcf_format")
        refused(fmt(slab=None), "no bv_engine_text_submit")
        # NULL arguments, reserved_
        refused(fmt(lines=False), "null")
        refused(fmt(out=None), "null")
        for k in ("site", "head_off", "gt", "head"):
            refused(fmt(**{k: None}), "null")
        refused(fmt(reserved=1), "reserved_")
        refused(fmt(head_off=np.array([0, 5, 2, 9], np.uint64)), "head_off out of order")
        for ch in b"5x/\x00":
            g = gt.copy(); g[6] = ch
            refused(fmt(gt=g), "gt of line 1")
        refused(fmt(site=np.array([0, R, 1], np.uint32)), "beyond the 4 rows")
        # the slab, as bv_engine_submit checks its planes
        def slab_with(**kw):
            s = P.slab(False)
            for k, v in kw.items():
                setattr(s, k, v)
            return s
        for s, word in ((slab_with(pitch=96), "pitch"), (slab_with(pitch=120), "pitch"), (slab_with(n_samples=0), "pitch"),
                        (slab_with(base_strand=None), "planes are required"), (slab_with(qual=None), "planes are required"),
                        (slab_with(qual=P.host[1][1].ctypes.data + 4), "16-byte aligned"), (slab_with(mem_kind=7), "mem_kind"),
                        (slab_with(layout=0x80), "layout"), (slab_with(reserved_=1), "layout"), (slab_with(n_sites=3), "beyond the 3 rows")):
            refused(fmt(slab=s), word)
        # a format, then a fetch without room and with a wrong kind; a deflate that bv_engine_bgzf_deflate_level refuses
        lines = make_lines(rng, site.tolist(), [2, 3, 4])
        heads, gt_ok, text, off = expected(harness, tmp_path, cell, phred, lines)
        got_off = eng.vcf_format(site, heads, gt_ok, P.slab(False))
        assert np.array_equal(got_off, off)
        refused(lib.bv_engine_vcf_fetch(h, dst.ctypes.data, len(text) - 1, _capi.BV_MEM_HOST, None), "dst_capacity")
        refused(lib.bv_engine_vcf_fetch(h, dst.ctypes.data, dst.size, 5, None), "dst_mem_kind")
        refused(lib.bv_engine_vcf_fetch(h, None, dst.size, _capi.BV_MEM_HOST, None), "null dst")
        boff = np.array([0, len(text) + 1], np.uint64)
        refused(lib.bv_engine_vcf_deflate(h, boff.ctypes.data, 1, 0, dst.ctypes.data, dst.size, moff.ctypes.data, None), "beyond text_bytes")
        boff = np.array([0, len(text)], np.uint64)
        refused(lib.bv_engine_vcf_deflate(h, boff.ctypes.data, 1, 9, dst.ctypes.data, dst.size, moff.ctypes.data, None), "level")
        refused(lib.bv_engine_vcf_deflate(h, boff.ctypes.data, 1, 0, dst.ctypes.data, len(text) + 30, moff.ctypes.data, None), "dst_capacity")
        # a refused format has touched nothing: the text of the last one is still there, and the engine still formats
        refused(fmt(reserved=1), "reserved_")
        assert eng.vcf_fetch().tobytes() == text
        assert format_and_fetch(eng, site, heads, gt_ok, P.slab(True))[1] == text
    finally:
        eng.close()


@pytest.mark.parametrize("via", ["lrt_text", "lrt_bgzf"])
def test_rows_kept_by_the_text_path(harness, tmp_path, via):
    """slab = NULL: the lines of every variant record of a parsed batch, from the rows bv_engine_text_submit left on the device.
    Two positions are skipped (Depth 0) and one is left to the host reader, so a record's index is not its position's and a
    host row stands among the parsed ones.  Expected: the harness's lines over the TextBatch's own cell and phred planes."""
    from basevar_amd import _capi
    from basevar_amd.synth import make_slab
    from test_gpu_text_rows import _py_host_reader, slab_rows
    from test_gpu_bgzf_rows import file_texts, members_of
    fs = [200, 120, 37]
    P, N, F = 30, sum(fs), 3
    slab = make_slab(P, N, seed=309, coverage=0.1, indel_frac=0.02, n_groups=2)
    text, off = slab_rows(slab, fs, depth_zero=(2, 11))
    rows = [[bytes(text[int(off[p * F + f]):int(off[p * F + f + 1]) - 1]) for f in range(F)] for p in range(P)]

    def sign_mapq(row):  # "+60": the host reader takes the sign, the device does not
        c = row.split(b"\t")
        c[4] = b" ".join(b"+" + t for t in c[4].split(b" "))
        return b"\t".join(c)
    rows[5] = [sign_mapq(r) for r in rows[5]]
    eng = engine(P, N)
    try:
        if via == "lrt_text":
            tb = eng.lrt_text(rows, fs, group_id=slab["group_id"], n_groups=2, host_reader=_py_host_reader(N))
        else:
            flat = b"".join(r + b"\n" for pos in rows for r in pos)
            roff = np.zeros(P * F + 1, np.uint64)
            roff[1:] = np.cumsum([len(r) + 1 for pos in rows for r in pos])
            runs = [members_of(t, 0x1000) for t in file_texts(np.frombuffer(flat, np.uint8), roff, P, F)]
            tb = eng.lrt_bgzf(runs, fs, group_id=slab["group_id"], n_groups=2, host_reader=_py_host_reader(N))
        assert (tb.row_state[[2, 11]] == _capi.BV_TEXT_SKIP).all() and (tb.row_state[5] == _capi.BV_TEXT_HOST).all()
        assert len(tb.sites) == P - 2 and 5 in tb.positions.tolist()
        variant = np.nonzero((tb.sites["status"] & _capi.BV_SITE_VARIANT) != 0)[0]
        assert variant.size >= 3 and (tb.positions[variant] != variant).any()
        if 5 not in tb.positions[variant].tolist():  # the host's row is formatted whether or not it was called variant
            variant = np.sort(np.append(variant, tb.positions.tolist().index(5)))
        names = [b"G0", b"G1"]
        lines = []
        for r in variant.tolist():
            p = int(tb.positions[r])
            c = rows[p][0].split(b"\t")
            rec = tb.sites[r].copy()
            if rec["n_alt"] == 0:  # (only the host's row can come here: give it an ALT, the harness formats variant records)
                rec["n_alt"], rec["alt"][0] = 1, 1
            lines.append(vr.line(r, rec, tb.groups[r], ref_base=c[2], ref_pos=int(c[1]), ref_id=c[0]))
        heads, gt, exp_text, exp_off = expected(harness, tmp_path, tb.cell, tb.phred, lines, names)
        got_off, got = format_and_fetch(eng, variant, heads, gt, None)
        assert np.array_equal(got_off, exp_off) and got == exp_text
        # a record index beyond the records is refused, and the rows are still there afterwards
        with pytest.raises(RuntimeError, match="beyond the %d records" % len(tb.sites)):
            eng.vcf_format([len(tb.sites)], heads[:1], gt[:1], None)
        assert format_and_fetch(eng, variant[::-1].copy(), heads[::-1], gt[::-1].copy(), None)[1] == b"".join(
            exp_text[int(exp_off[k]):int(exp_off[k + 1])] for k in range(len(variant) - 1, -1, -1))
    finally:
        eng.close()
