"""GPU tests of bv_engine_pileup_text / _fetch / _deflate (include/basevar_amd_pileup_text.h), all through the C ABI: the text the
device writes is, byte for byte, that of the serial restatement pileup_text_model.rows_text and of the stand-alone harness
tests/cpp/pileup_text_check.cpp (the core of basevar_amd/csrc/bv_pileup_text_core.h, held to host/pileup.hpp's pileup_rows_text
inside the harness) -- at the sample counts, row counts, coverages, value and alignment edges at which the kernels of
basevar_amd/csrc/bv_pileup_text.hip can go wrong."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pileup_raw_cases as rc  # noqa: E402
import pileup_ref as pr  # noqa: E402
import pileup_text_model as ptm  # noqa: E402

SENTINEL = 0xA5
N_MAX = 300


def tile_samples():
    from basevar_amd import _capi
    return int(_capi.load().bv_pileup_text_tile_samples())


T = None  # BV_PTEXT_TILE, read once (tile())


def tile():
    global T
    if T is None:
        T = tile_samples()
    return T


@pytest.fixture(scope="module")
def harness():
    return ptm.build(asan=False)


@pytest.fixture(scope="module")
def eng():
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=1024, min_af_value=bv.min_af(N_MAX), device=0, max_samples=4096)
    yield e
    e.close()


def aligned(a):
    """a copy of the array at a 64-byte aligned address"""
    raw = np.zeros(a.nbytes + 64, np.uint8)
    at = (-raw.ctypes.data) % 64
    out = raw[at:at + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def as_arg(t, device=False):
    import torch
    tok, text = t.token_arrays()
    planes = dict(cell=aligned(t.cell), qual=aligned(t.qual), mapq=aligned(t.mapq), rank=aligned(t.rank))
    if device:
        planes = {k: torch.from_numpy(v).cuda() for k, v in planes.items()}
        torch.cuda.synchronize()
    return dict(planes, beg=t.beg, n_samples=t.n, tokens=tok, text=text)


def device_text(eng, t, first=0, n=None, device=False, chrom=None):
    eng.pileup_set_reference(t.ref)
    off = eng.pileup_text(chrom if chrom is not None else t.chrom, first, n, tile=as_arg(t, device))
    text = eng.pileup_text_fetch().tobytes()
    assert int(off[0]) == 0 and len(text) == int(off[-1])
    return text, off


def same_as_model(eng, t, harness=None, tmp=None, **kw):
    text, off = device_text(eng, t, **kw)
    want, want_off = ptm.rows_text(t, kw.get("first", 0), kw.get("n"))
    assert (off == want_off).all()
    if text != want:
        at = next(i for i in range(min(len(text), len(want))) if text[i] != want[i])
        raise AssertionError("texts differ at byte %d of %d: device %r, model %r" % (at, len(want), text[max(0, at - 30):at + 30], want[max(0, at - 30):at + 30]))
    if harness is not None:
        assert ptm.run_tile(harness, tmp, t, kw.get("first", 0), kw.get("n"))[0] == text
    return text, off


# ----------------------------------------------------------------------------------------------------- 1. sample counts, explicit tiles
def sample_counts():
    t = tile()
    return [1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1]


@pytest.mark.parametrize("k", range(9))
def test_sample_counts_rows_and_coverages(eng, harness, tmp_path, k):
    """n = 1, 2, 63, 64, 65, T-1, T, T+1, 2T+1 by rows = 1, 2, 64, 65 by coverage 0, 0.08, 0.5, 1; host and device planes; a pitch 48
    wider than needed, with random bytes in the padding"""
    n = sample_counts()[k]
    combos = [(1, 1.0, False, 0), (2, 0.0, True, 48), (64, 0.08, True, 0), (65, 0.5, False, 48), (1, 0.08, True, 48), (2, 0.5, True, 0)]
    for j, (rows, cov, device, extra) in enumerate(combos):
        t = ptm.random_tile(100 * k + j, n, rows, cov, beg=1 + 37 * j, pitch_extra=extra, long_tokens=(63, 64, 65, 129, 200) if j == 3 else ())
        assert t.pitch == (n + 15) // 16 * 16 + extra
        same_as_model(eng, t, harness if j in (0, 3) else None, tmp_path, device=device)


def test_all_placeholder_rows_between_covered_ones(eng):
    """steps of 64 samples without a claimed cell beside steps with them, in one tile and across tiles"""
    t = ptm.random_tile(7, 2 * tile() + 70, 5, 1.0)
    t.rank[:, 64:192] = 0
    t.rank[1, :] = 0
    t.rank[3, tile():2 * tile()] = 0
    t.tokens = {k: v for k, v in t.tokens.items() if t.rank[k[0] - t.beg, k[1]]}
    same_as_model(eng, t)


# ------------------------------------------------------------------------------------------------------------------ 2. value edges
def test_value_edges_of_mapq_rank_quality_and_depth(eng, harness, tmp_path):
    n = 256
    rng = np.random.default_rng(3)
    mapqs, ranks = [0, 9, 10, 99, 100, 255], [1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535]
    depths = [0, 1, 9, 10, 99, 100, 255, 256]
    rows = len(depths) + 1
    cell = rng.integers(0, 8, (rows, n), dtype=np.uint8)
    mapq = np.array(mapqs, np.uint8)[rng.integers(0, len(mapqs), (rows, n))]
    rank = np.array(ranks, np.uint16)[rng.integers(0, len(ranks), (rows, n))]
    qual = np.tile(np.arange(n, dtype=np.uint8), (rows, 1))  # every quality 0 .. 255 in every row
    for r, d in enumerate(depths):
        rank[r, rng.permutation(n)[d:]] = 0
    t = ptm.Tile(b"chrV", 95, n, cell, qual, mapq, rank, {}, bytes(rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8), 200)))
    text, off = same_as_model(eng, t, harness, tmp_path)
    assert [int(text[int(off[r]):int(off[r]) + 40].split(b"\t")[3]) for r in range(len(depths))] == depths
    for m in mapqs:
        assert (mapq[rank != 0] == m).any()
    for k in ranks:
        assert (rank == k).any()


@pytest.mark.parametrize("edge", [9, 99, 999, 9999, 99999, 500000])
def test_positions_across_a_digit_edge(eng, edge):
    """9|10 ... 99,999|100,000 and the 500,000|500,001 step edge"""
    t = ptm.random_tile(edge, 70, 4, 0.5, beg=edge - 1)
    text, off = same_as_model(eng, t, device=True)
    assert text[int(off[1]):].startswith(b"chr7\t%d\t" % edge) and text[int(off[2]):].startswith(b"chr7\t%d\t" % (edge + 1))


def test_chrom_of_1_to_40_bytes_and_the_alignment_census(eng):
    """every CHROM length 1 .. 40 over a tile of T + 5 samples; and from the EXPECTED text: a line start, each of the five list
    starts and a tile boundary inside each list fall on all 16 residues modulo 16"""
    t = ptm.random_tile(11, tile() + 5, 3, 0.3, long_tokens=(2, 3, 63, 64, 65, 129, 200))
    line, lists, cuts = set(), [set() for _ in range(5)], [set() for _ in range(5)]
    for ln in range(1, 41):
        t.chrom = (b"chromosome_with_a_long_name_0123456789_xyz")[:ln]
        same_as_model(eng, t, device=ln % 2 == 0)
        places, total = ptm.row_places(t, tile())
        assert total == len(ptm.rows_text(t)[0])
        for at, starts, cut in places:
            line.add(at % 16)
            for l in range(5):
                lists[l].add(starts[l] % 16)
                assert len(cut[l]) == 1
                cuts[l].add(cut[l][0] % 16)
    every = set(range(16))
    assert line == every and all(s == every for s in lists) and all(c == every for c in cuts)


def test_token_lengths_and_places(eng, harness, tmp_path):
    """tokens of 2, 3, 63, 64, 65, 129 and 200 bytes in the first and the last sample of a tile and in neighbouring samples; a step
    whose tokens exceed the kernel's image; one token longer than it"""
    n = tile() + 66
    lens = [2, 3, 63, 64, 65, 129, 200]
    rows = len(lens) + 2
    rng = np.random.default_rng(4)
    pitch = (n + 15) // 16 * 16
    cell = rng.integers(0, 8, (rows, pitch), dtype=np.uint8)
    rank = np.ones((rows, pitch), np.uint16)
    rank[rng.random((rows, pitch)) < 0.5] = 0
    tokens = {}
    beg = 40

    def put(r, s, ln):
        cell[r, s] = ptm.CELL_INS if (r + s) % 2 else ptm.CELL_DEL | ptm.CELL_REV
        rank[r, s] = 1 + s
        tokens[(beg + r, s)] = (b"+" if (r + s) % 2 else b"-") + bytes(rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), ln - 1))

    for r, ln in enumerate(lens):
        for s in (0, 1, 2, 63, 64, tile() - 2, tile() - 1, tile(), tile() + 1, n - 1):
            put(r, s, ln)
    for s in range(128, 192):      # 64 x 200 bytes in one step
        put(len(lens), s, 200)
    put(len(lens) + 1, 5, 9000)    # longer than the image, twice
    put(len(lens) + 1, 6, 2)
    t = ptm.Tile(b"chrT", beg, n, cell, np.full((rows, pitch), 30, np.uint8), np.full((rows, pitch), 60, np.uint8), rank, tokens,
                 bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 100)))
    same_as_model(eng, t, harness, tmp_path)
    same_as_model(eng, t, device=True, first=len(lens), n=2)


# ---------------------------------------------------------------------------------------------------------- 3. from a pileup (tile=None)
@pytest.fixture(scope="module")
def pileup_harness():
    return pr.build()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return pr.Corpus(tmp_path_factory.mktemp("ptext_corpus"), N_MAX)


def pile(eng, d, window):
    return eng.pileup(d.records, d.run_off, d.run_sample, d.n_samples, d.tid, pr.REGION, window, pr.MAPQ_THD)


@pytest.mark.parametrize("n", [1, 65, N_MAX])
def test_text_of_the_last_pileup(eng, pileup_harness, corpus, tmp_path, n):
    """the corpus at windows w1, w64, w65, w1000 and edge: planes, depths, tokens and token text are read where the pileup left them"""
    eng.pileup_set_reference(corpus.fa)
    for name in ("w1", "w64", "w65", "w1000", "edge"):
        window = pr.WINDOWS[name]
        d = pr.run_bam(pileup_harness, tmp_path / "d.bin", corpus, n, window)[0]
        t = ptm.from_dump(d, pr.REF_ID, corpus.fa, window[0])
        pile(eng, d, window)
        off = eng.pileup_text(pr.REF_ID)
        want, want_off = ptm.rows_text(t)
        assert (off == want_off).all() and eng.pileup_text_fetch().tobytes() == want, name
        if name == "w1000":
            assert len(t.tokens) >= 4 and max(len(v) for v in t.tokens.values()) > 64


def test_hand_built_raw_cases(eng, pileup_harness, tmp_path):
    """tests/pileup_raw_cases.py: operation codes 0-15, quals 0-255, long token texts"""
    done = 0
    for name, c in sorted(rc.directed().items()):
        if c.status:
            continue
        d = pr.run_raw(pileup_harness, tmp_path / "d.bin", tmp_path, c.ref, c.runs, c.run_sample, c.n_samples, c.window)[0]
        t = ptm.from_dump(d, b"chr1", c.ref, c.window[0])
        eng.pileup_set_reference(c.ref)
        eng.pileup(b"".join(c.runs), d.run_off, c.run_sample, c.n_samples, pr.TID, pr.REGION, c.window, pr.MAPQ_THD)
        off = eng.pileup_text("chr1")
        want, want_off = ptm.rows_text(t)
        assert (off == want_off).all() and eng.pileup_text_fetch().tobytes() == want, name
        done += 1
    assert done >= 7


def test_a_pileup_without_runs(eng, corpus):
    eng.pileup_set_reference(corpus.fa)
    n, window = 70, (1300, 1363)
    assert eng.pileup(b"", np.zeros(1, np.uint64), np.zeros(0, np.uint32), n, pr.TID, pr.REGION, window, pr.MAPQ_THD) == 0
    off = eng.pileup_text("chr1")
    want = b"".join(b"chr1\t%d\t%s\t0\t" % (p, corpus.fa[p - 1:p].encode()) + b"\t".join(b" ".join([x] * n) for x in (b"0", b"N", b"!", b"0", b".")) + b"\n"
                    for p in range(window[0], window[1] + 1))
    assert eng.pileup_text_fetch().tobytes() == want and int(off[-1]) == len(want)


def submit_records(eng):
    from basevar_amd import _capi
    slab, pos, depth = eng.pileup_rows()
    out = np.zeros(int(slab.n_sites), _capi.SITE_DTYPE)
    rc_ = eng._lib.bv_engine_pileup_submit(eng._h, 0, int(slab.n_sites), None, 0, out.ctypes.data, None, None, None, None)
    assert rc_ == 0, eng._err()
    return out.tobytes(), pos.tobytes(), depth.tobytes()


def test_the_pileup_stays_usable_by_rows_and_submit(eng, pileup_harness, corpus, tmp_path):
    eng.pileup_set_reference(corpus.fa)
    window = pr.WINDOWS["w1000"]
    d = pr.run_bam(pileup_harness, tmp_path / "d.bin", corpus, 65, window)[0]
    pile(eng, d, window)
    before = submit_records(eng)
    eng.pileup_text(pr.REF_ID)
    text = eng.pileup_text_fetch().tobytes()
    assert submit_records(eng) == before and len(before[0]) > 0
    eng.pileup_text(pr.REF_ID, 10, 5)
    assert submit_records(eng) == before
    assert eng.pileup_fetch()["cell"][:, :65].tobytes() == d.cell[:, :65].tobytes()
    eng.pileup_text(pr.REF_ID)
    assert eng.pileup_text_fetch().tobytes() == text


def test_the_consumer_reads_the_rows_the_device_wrote(pileup_harness, corpus, tmp_path):
    """the rows written for w1000 at 65 samples, fed to lrt_text, give the records of lrt_pileup over the same window for every
    covered position.  Two rows of the corpus cannot be read back by any batchfile reader, whichever writer wrote them: the indels
    of its empty reads have quality 255, written as the byte 0x20, a space inside the quality list.  The device parser hands such
    rows to the host reader, the suite's tolerant one skips them; they are exactly the rows with that byte, and nothing else is
    skipped."""
    import basevar_amd as bv
    from test_gpu_bgzf_rows import tolerant_reader
    n, window = 65, pr.WINDOWS["w1000"]
    d = pr.run_bam(pileup_harness, tmp_path / "d.bin", corpus, n, window)[0]
    e = bv.BaseTypeEngine(max_sites=1024, min_af_value=bv.min_af(n), device=0, max_samples=n)
    e.pileup_set_reference(corpus.fa)
    want = e.lrt_pileup(d.records, d.run_off, d.run_sample, n, d.tid, pr.REGION, window, pr.MAPQ_THD)
    off = e.pileup_text(pr.REF_ID)
    text = e.pileup_text_fetch()
    got = e.lrt_text((text, off), [n], host_reader=tolerant_reader(n))
    spaced = {int(p) for p in np.unique(np.nonzero((d.qual[:, :n] == 255) & (d.rank[:, :n] != 0))[0])}
    covered = [int(p) - window[0] for p in want.positions]
    assert spaced and spaced <= set(covered) and len(spaced) <= 4
    assert [int(p) for p in got.positions] == [p for p in covered if p not in spaced]
    keep = np.array([p not in spaced for p in covered])
    assert got.sites.tobytes() == want.sites[keep].tobytes() and len(got.sites) > 900
    e.close()


# ------------------------------------------------------------------------------------------------------------------ 4. sub-ranges
def test_sub_ranges_reproduce_slices_of_the_whole(eng, pileup_harness, corpus, tmp_path):
    t = ptm.random_tile(21, tile() + 3, 33, 0.3, long_tokens=(200, 129, 65))
    whole, off = same_as_model(eng, t)
    ranges = [(32, 1), (20, 10), (15, 10), (10, 10), (0, 1), (5, 0), (33, 0), (0, 33), (31, 2)]  # reversed, overlapping, single rows, the last row, n = 0
    for device in (False, True):
        for first, n in ranges:
            part, part_off = device_text(eng, t, first, n, device=device)
            assert part == whole[int(off[first]):int(off[first + n])] and (part_off == off[first:first + n + 1] - off[first]).all()
            assert part_off.size == n + 1
    # ... and of the last pileup
    eng.pileup_set_reference(corpus.fa)
    window = pr.WINDOWS["w65"]
    d = pr.run_bam(pileup_harness, tmp_path / "d.bin", corpus, 65, window)[0]
    pile(eng, d, window)
    off = eng.pileup_text(pr.REF_ID)
    whole = eng.pileup_text_fetch().tobytes()
    for first, n in [(64, 1), (40, 20), (30, 20), (0, 1), (65, 0), (7, None)]:
        part_off = eng.pileup_text(pr.REF_ID, first, n)
        n = 65 - first if n is None else n
        assert eng.pileup_text_fetch().tobytes() == whole[int(off[first]):int(off[first + n])] and int(part_off[-1]) == int(off[first + n] - off[first])


# ----------------------------------------------------------------------------------------------------------------------- 5. fetch
def test_fetch_touches_nothing_around_its_destination(eng):
    import torch
    from basevar_amd import _capi
    t = ptm.random_tile(31, 130, 9, 0.4)
    text, _ = device_text(eng, t)
    size, pad = len(text), 64
    host = np.full(size + 2 * pad, SENTINEL, np.uint8)
    assert eng._lib.bv_engine_pileup_text_fetch(eng._h, host[pad:].ctypes.data, size, _capi.BV_MEM_HOST, None) == 0
    assert host[pad:pad + size].tobytes() == text and (host[:pad] == SENTINEL).all() and (host[pad + size:] == SENTINEL).all()
    dev = torch.full((size + 2 * pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert eng.pileup_text_fetch(int(dev.data_ptr()) + pad, size) is None
    back = dev.cpu().numpy()
    assert back[pad:pad + size].tobytes() == text and (back[:pad] == SENTINEL).all() and (back[pad + size:] == SENTINEL).all()
    # one byte short: refused, nothing written
    host[:] = SENTINEL
    assert eng._lib.bv_engine_pileup_text_fetch(eng._h, host[pad:].ctypes.data, size - 1, _capi.BV_MEM_HOST, None) == _capi.BV_ERR_INVALID_ARG
    assert b"dst_capacity %d < the text's %d bytes" % (size - 1, size) in eng._lib.bv_last_error(eng._h) and (host == SENTINEL).all()
    dev.fill_(SENTINEL)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="dst_capacity"):
        eng.pileup_text_fetch(int(dev.data_ptr()) + pad, size - 1)
    assert (dev.cpu().numpy() == SENTINEL).all()
    assert eng._lib.bv_engine_pileup_text_fetch(eng._h, host.ctypes.data, size, 7, None) == _capi.BV_ERR_INVALID_ARG
    assert eng._lib.bv_engine_pileup_text_fetch(eng._h, None, size, _capi.BV_MEM_HOST, None) == _capi.BV_ERR_INVALID_ARG


# --------------------------------------------------------------------------------------------------------------------- 6. deflate
def inflate_members(members, member_off):
    out = []
    for k in range(len(member_off) - 1):
        m = members[int(member_off[k]):int(member_off[k + 1])].tobytes()
        out.append(zlib.decompress(m, 31))
    return b"".join(out)


@pytest.mark.parametrize("level", ["fast", "small"])
def test_deflate_gives_the_members_of_the_fetched_text(eng, level):
    t = ptm.random_tile(41, 300, 120, 0.08)
    text, off = device_text(eng, t)
    assert len(text) > 2 * 0xff00
    members, member_off = eng.pileup_text_deflate(level=level)
    want, want_off = eng.bgzf_deflate(text, level=level)
    assert members.tobytes() == want.tobytes() and (member_off == want_off).all() and member_off.size >= 4
    assert inflate_members(members, member_off) == text
    # blocks of the caller's choice: a block per row group
    block_off = off[::7].copy()
    block_off[-1] = off[-1]
    members, member_off = eng.pileup_text_deflate(block_off=block_off, level=level)
    want, want_off = eng.bgzf_deflate(text, block_off=block_off, level=level)
    assert members.tobytes() == want.tobytes() and (member_off == want_off).all()
    assert inflate_members(members, member_off) == text


# ------------------------------------------------------------------------------------------------- 7. the reference's own rows
def test_golden_rows_on_the_device(eng):
    """the parsed rounds of tests/golden/reference_pileup_rows.txt.gz as explicit tiles give the file's bytes"""
    rounds = ptm.golden_rounds()
    assert len(rounds) == 60
    for r, want in rounds:
        t = ptm.parse_rows(want)
        text, _ = device_text(eng, t, device=r % 2 == 1)
        assert text == want, r


# ------------------------------------------------------------------------------------------------------------------- 8. refusals
def refused(eng, status, message, chrom, first=0, n=None, tile=None, **patch):
    """bv_engine_pileup_text with fields of its argument patched: the status, the message, and no text afterwards"""
    from basevar_amd import _capi
    with pytest.raises(RuntimeError) as ei:
        if patch:
            arg = dict(tile)
            arg.update(patch)
            eng.pileup_text(chrom, first, n, tile=arg)
        else:
            eng.pileup_text(chrom, first, n, tile=tile)
    assert ei.value.args[1] == status and message in str(ei.value), str(ei.value)
    with pytest.raises(RuntimeError, match="no bv_engine_pileup_text before it"):
        eng.pileup_text_fetch()
    with pytest.raises(RuntimeError, match="no bv_engine_pileup_text before it"):
        eng.pileup_text_deflate()
    assert _capi.BV_ERR_INVALID_ARG == -1


def test_refusals(harness, tmp_path):
    import basevar_amd as bv
    from basevar_amd import _capi
    INV, DATA = _capi.BV_ERR_INVALID_ARG, _capi.BV_ERR_DATA
    e = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(100), device=0, max_samples=256)
    t = ptm.random_tile(51, 70, 6, 0.6, beg=100)
    arg = as_arg(t)
    L = e._lib
    row_off = np.zeros(8, np.uint64)
    req = _capi.PileupText(None, b"c", 1, 0, 1, 0)
    assert L.bv_engine_pileup_text(e._h, None, row_off.ctypes.data, None) == INV and b"null in/row_off" in L.bv_last_error(e._h)
    assert L.bv_engine_pileup_text(e._h, C.byref(req), None, None) == INV and b"null in/row_off" in L.bv_last_error(e._h)
    req.reserved_ = 1
    assert L.bv_engine_pileup_text(e._h, C.byref(req), row_off.ctypes.data, None) == INV and b"reserved_ must be zero" in L.bv_last_error(e._h)
    # no reference set; no completed pileup
    refused(e, INV, "no reference set", "c", tile=arg)
    refused(e, INV, "no completed bv_engine_pileup", "c")
    e.pileup_set_reference(t.ref)
    refused(e, INV, "no completed bv_engine_pileup", "c")
    assert e.pileup_text("c", tile=arg)[-1] > 0  # (the tile itself is fine)
    # chrom
    refused(e, INV, "chrom must have 1 to 255 bytes", b"", tile=arg)
    refused(e, INV, "chrom must have 1 to 255 bytes", b"c" * 256, tile=arg)
    assert e.pileup_text(b"c" * 255, 0, 1, tile=arg)[-1] > 255
    refused(e, INV, "chrom must not hold a tab", b"c\tx", tile=arg)
    refused(e, INV, "chrom must not hold a tab", b"c\nx", tile=arg)
    # the tile: mem_kind, pitch, alignment, NULL planes
    refused(e, INV, "mem_kind must be", "c", tile=arg, mem_kind=2)
    refused(e, INV, "pitch must be", "c", tile=arg, pitch=t.pitch + 8)
    refused(e, INV, "pitch must be", "c", tile=arg, n_samples=t.pitch + 1)
    refused(e, INV, "pitch must be", "c", tile=arg, n_samples=0)
    odd = np.zeros(t.cell.size + 128, np.uint8)
    odd = odd[(-odd.ctypes.data) % 64 + 8:][:t.cell.size].reshape(t.cell.shape)
    refused(e, INV, "planes must be 16-byte aligned", "c", tile=arg, qual=odd)
    # rows beyond the tile, beyond the reference
    refused(e, INV, "are beyond the tile's 6", "c", 6, 1, tile=arg)
    refused(e, INV, "are beyond the tile's 6", "c", 0, 7, tile=arg)
    e.pileup_set_reference(t.ref[:103])
    refused(e, INV, "beyond the reference's 103 bases", "c", tile=arg)
    assert e.pileup_text("c", 0, 4, tile=arg)[-1] > 0
    e.pileup_set_reference(t.ref)
    # tokens out of order, out of bounds
    tok, text = t.token_arrays()
    assert tok.size >= 4
    swapped = tok.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    refused(e, INV, "strictly ascending by (pos, sample): token 2", "c", tile=arg, tokens=swapped)
    twice = tok.copy()
    twice[3] = twice[2]
    refused(e, INV, "strictly ascending by (pos, sample): token 3", "c", tile=arg, tokens=twice)
    far = tok.copy()
    far[1]["text_len"] = text.size
    refused(e, INV, "the text of token 1 lies beyond text_bytes", "c", tile=arg, tokens=far)
    far = tok.copy()
    far[0]["text_off"] = 2 ** 63
    refused(e, INV, "the text of token 0 lies beyond text_bytes", "c", tile=arg, tokens=far)
    # BV_ERR_DATA: an indel cell without a token -- a deliberately inconsistent tile; the count pass finds it, nothing is written
    key = sorted(t.tokens)[len(t.tokens) // 2]
    short = ptm.Tile(t.chrom, t.beg, t.n, t.cell, t.qual, t.mapq, t.rank, {k: v for k, v in t.tokens.items() if k != key}, t.ref)
    assert ptm.run_tile(harness, tmp_path, short) == ("missing",) + key
    for device in (False, True):
        refused(e, DATA, "the indel cell at pos %d, sample %d has no token" % key, "c", tile=as_arg(short, device))
    row = key[0] - t.beg
    if row + 1 < t.rows:  # the rows behind it are complete
        assert e.pileup_text(short.chrom, row + 1, t.rows - row - 1, tile=as_arg(short))[-1] == len(ptm.rows_text(short, row + 1, t.rows - row - 1)[0])
    # n = 0: an empty text
    assert e.pileup_text("c", 3, 0, tile=arg).tolist() == [0] and e.pileup_text_fetch().size == 0
    members, member_off = e.pileup_text_deflate()
    assert members.size == 0 and member_off.tolist() == [0]
    e.close()
