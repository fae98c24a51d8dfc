"""GPU tests of bv_engine_pileup_text_parts (include/basevar_amd_pileup_text_parts.h) through the C ABI: the text the device writes
for sample parts of a tile is, byte for byte, pileup_text_model.rows_text applied to the column-sliced planes with tokens rebased
(pileup_text_parts_model.parts_text) and the dump of the stand-alone harness tests/cpp/pileup_text_parts_check.cpp (which holds
the core's definition to host/pileup.hpp's pileup_rows_text on the sliced tile) -- at the part sizes, start residues, tile
boundaries, row counts, coverages, token places and alignments at which the kernels of basevar_amd/csrc/bv_pileup_text_parts.hip
can go wrong.  Every fetched text lands between sentinels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pileup_ref as pr  # noqa: E402
import pileup_text_model as ptm  # noqa: E402
import pileup_text_parts_model as ppm  # noqa: E402
from test_gpu_pileup_text import as_arg, inflate_members, submit_records, tile  # noqa: E402

SENTINEL, PAD = 0xA5, 64
RESIDUES = (0, 1, 8, 15)


@pytest.fixture(scope="module")
def harness():
    return ppm.build(asan=False)


@pytest.fixture(scope="module")
def eng():
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=1024, min_af_value=bv.min_af(300), device=0, max_samples=4096)
    yield e
    e.close()


def fetch_between_sentinels(eng, size):
    from basevar_amd import _capi
    host = np.full(size + 2 * PAD, SENTINEL, np.uint8)
    assert eng._lib.bv_engine_pileup_text_fetch(eng._h, host[PAD:].ctypes.data, size, _capi.BV_MEM_HOST, None) == 0, eng._err()
    assert (host[:PAD] == SENTINEL).all() and (host[PAD + size:] == SENTINEL).all()
    return host[PAD:PAD + size].tobytes()


def device_parts(eng, t, part_first, first=0, n=None, device=False, arg=None):
    eng.pileup_set_reference(t.ref)
    off = eng.pileup_text_parts(t.chrom, part_first, first, n, tile=arg if arg is not None else as_arg(t, device))
    assert int(off[0]) == 0
    return fetch_between_sentinels(eng, int(off[-1])), off


def same_as_model(eng, t, part_first, harness=None, tmp=None, **kw):
    text, off = device_parts(eng, t, part_first, **kw)
    want, want_off = ppm.parts_text(t, part_first, kw.get("first", 0), kw.get("n"))
    assert off.size == want_off.size and (off == want_off).all()
    if text != want:
        at = next(i for i in range(min(len(text), len(want))) if text[i] != want[i])
        raise AssertionError("texts differ at byte %d of %d: device %r, model %r" % (at, len(want), text[max(0, at - 30):at + 30], want[max(0, at - 30):at + 30]))
    if harness is not None:
        dump, dump_off = ppm.run_parts(harness, tmp, t, part_first, kw.get("first", 0), kw.get("n"))
        assert dump == text and (dump_off == off).all()
    return text, off


# ------------------------------------------------------------------------------------------------------- 1. part sizes and starts
def part_sizes():
    t = tile()
    return [1, 2, 63, 64, 65, 200, t - 1, t, t + 1, 2 * t + 1]


@pytest.mark.parametrize("k", range(10))
def test_part_sizes_at_every_start_residue(eng, harness, tmp_path, k):
    """sizes 1, 2, 63, 64, 65, 200, T-1, T, T+1, 2T+1, each starting at column residues 0, 1, 8, 15 modulo 16 (behind one whole word,
    so that columns lie before it too), alone and with neighbour parts on both sides; host and device planes"""
    size = part_sizes()[k]
    rows = [1, 2, 64, 65, 2, 3, 5, 2, 3, 2][k]
    n = 16 + 15 + size + 9
    t = ptm.random_tile(300 + k, n, rows, [1.0, 0.5, 0.08, 0.5, 0.08, 0.3, 0.5, 0.08, 0.5, 0.3][k], beg=1 + 31 * k, pitch_extra=48 if k % 2 else 0,
                        long_tokens=(63, 64, 65, 129, 200) if k in (3, 5, 9) else ())
    for j, r in enumerate(RESIDUES):
        s0 = 16 + r
        same_as_model(eng, t, [s0, s0 + size], harness if j == 1 else None, tmp_path, device=j % 2 == 1)
    same_as_model(eng, t, [0, 16 + 8, 16 + 8 + size, n], harness, tmp_path, device=k % 2 == 0)


def test_the_largest_shape(eng):
    """2T + 1 samples by 65 rows, as parts of 200 with a remainder"""
    n = 2 * tile() + 1
    t = ptm.random_tile(77, n, 65, 0.08)
    same_as_model(eng, t, list(range(0, n, 200)) + [n], device=True)


def test_parts_around_a_tile_boundary_of_the_planes(eng, harness, tmp_path):
    """parts that end before, on and behind a BV_PTEXT_TILE-column boundary of the planes, and parts that cross one: a part's tiles
    are counted from ITS first column"""
    T = tile()
    n = 2 * T + 40
    t = ptm.random_tile(78, n, 3, 0.3, long_tokens=(200, 129, 65, 64, 63))
    same_as_model(eng, t, [0, T - 1, T, T + 1, 2 * T - 5, 2 * T, 2 * T + 3, n], harness, tmp_path)
    same_as_model(eng, t, [T - 100, T + 100, 2 * T - 8, 2 * T + 8], device=True)   # crossing, 200 and 16 samples
    same_as_model(eng, t, [9, 9 + T + 1, 9 + 2 * T + 2], device=True)             # two tiles each, the second of one sample, crossing


# --------------------------------------------------------------------------------------------------------- 2. covering all samples
def test_one_part_of_all_samples_is_pileup_text(eng):
    for n in (1, 65, tile() + 5):
        t = ptm.random_tile(80 + n, n, 4, 0.4, long_tokens=(129, 2))
        arg = as_arg(t, device=n == 65)
        eng.pileup_set_reference(t.ref)
        off = eng.pileup_text(t.chrom, tile=arg)
        whole = eng.pileup_text_fetch().tobytes()
        text, poff = device_parts(eng, t, [0, n], arg=arg)
        assert text == whole == ptm.rows_text(t)[0] and (poff == off).all()


def test_batches_with_a_remainder_and_gaps(eng, harness, tmp_path):
    n = 450
    t = ptm.random_tile(91, n, 6, 0.3)
    text, off = same_as_model(eng, t, [0, 200, 400, n], harness, tmp_path)
    # the parts' depths add up to the whole row's (a row is not split at its line break: a quality byte may be one)
    for k in range(t.rows):
        assert sum(int(text[int(off[p * t.rows + k]):].split(b"\t", 4)[3]) for p in range(3)) == int((t.rank[k, :n] != 0).sum())
    # gaps before, behind, and -- as two calls -- between parts
    same_as_model(eng, t, [5, 100, 300], harness, tmp_path, device=True)
    same_as_model(eng, t, [5, 100], device=True)
    same_as_model(eng, t, [120, 300])
    same_as_model(eng, t, [449, 450])


# ----------------------------------------------------------------------------------------------------------------------- 3. rows
def test_row_counts_and_sub_ranges(eng):
    t = ptm.random_tile(92, 300, 65, 0.2, long_tokens=(200, 129))
    pf = [8, 208, 300]
    whole, off = same_as_model(eng, t, pf)
    for j, (first, cnt) in enumerate([(0, 1), (0, 2), (0, 64), (0, 65), (64, 1), (20, 10), (15, 10), (5, 0), (65, 0), (63, 2)]):
        text, poff = same_as_model(eng, t, pf, first=first, n=cnt, device=j % 2 == 1)
        assert poff.size == 2 * cnt + 1
        for p in range(2):
            a, b = int(off[p * 65 + first]), int(off[p * 65 + first + cnt])
            assert text[int(poff[p * cnt]):int(poff[(p + 1) * cnt])] == whole[a:b]


def test_coverage_0_and_1_and_a_row_claimed_only_outside_the_part(eng):
    for cov in (0.0, 1.0):
        same_as_model(eng, ptm.random_tile(93, 130, 3, cov), [1, 66, 129], device=cov == 0.0)
    t = ptm.random_tile(94, 100, 3, 1.0, indel_frac=0.0)
    t.rank[1, 24:57] = 0
    text, off = same_as_model(eng, t, [8, 24, 57, 100])
    row = text[int(off[3 + 1]):int(off[3 + 2])].split(b"\t")
    assert row[3] == b"0" and row[4] == b" ".join([b"0"] * 33) and row[5] == b" ".join([b"N"] * 33) and row[8] == b" ".join([b"."] * 33) + b"\n"
    assert text[int(off[1]):].split(b"\t", 4)[3] == b"16" and text[int(off[6 + 1]):].split(b"\t", 4)[3] == b"43"


# --------------------------------------------------------------------------------------------------------------------- 4. tokens
def token_tile(pf, lens, seed=4):
    """claimed indel cells with tokens of the given lengths at the first and last sample of every part, at the neighbouring
    parts' edge samples, and at the tile edges inside the parts"""
    T = tile()
    n = pf[-1] + 3
    rows = len(lens)
    rng = np.random.default_rng(seed)
    pitch = (n + 15) // 16 * 16
    cell = rng.integers(0, 8, (rows, pitch), dtype=np.uint8)
    rank = np.ones((rows, pitch), np.uint16)
    rank[rng.random((rows, pitch)) < 0.5] = 0
    tokens, beg = {}, 40
    places = set()
    for p in range(len(pf) - 1):
        places |= {pf[p], pf[p + 1] - 1}
        places |= {s for s in (pf[p] + T - 1, pf[p] + T, pf[p] + 2 * T - 1, pf[p] + 2 * T) if s < pf[p + 1]}
    places |= {s for s in (pf[0] - 1, pf[-1]) if 0 <= s < n}
    for r, ln in enumerate(lens):
        for s in sorted(places):
            cell[r, s] = ptm.CELL_INS if (r + s) % 2 else ptm.CELL_DEL | ptm.CELL_REV
            rank[r, s] = 1 + s % 60000
            tokens[(beg + r, s)] = (b"+" if (r + s) % 2 else b"-") + bytes(rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), ln - 1))
    t = ptm.Tile(b"chrT", beg, n, cell, np.full((rows, pitch), 30, np.uint8), np.full((rows, pitch), 60, np.uint8), rank, tokens,
                 bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 100)))
    return t, sorted(places)


def test_tokens_at_part_and_tile_edges(eng, harness, tmp_path):
    T = tile()
    pf = [7, 207, 207 + T + 1, 207 + T + 1 + 2 * T + 1]
    t, places = token_tile(pf, [2, 3, 64, 200, 9000])
    assert 6 in places and pf[-1] in places  # the neighbours of the first and the last part: in gaps, their tokens go nowhere
    same_as_model(eng, t, pf, harness, tmp_path)
    same_as_model(eng, t, pf, device=True, first=3, n=2)


def refused(eng, status, message, chrom, part_first, first=0, n=None, tile=None):
    with pytest.raises(RuntimeError) as ei:
        eng.pileup_text_parts(chrom, part_first, first, n, tile=tile)
    assert ei.value.args[1] == status and message in str(ei.value), str(ei.value)
    with pytest.raises(RuntimeError, match="no bv_engine_pileup_text before it"):
        eng.pileup_text_fetch()
    with pytest.raises(RuntimeError, match="no bv_engine_pileup_text before it"):
        eng.pileup_text_deflate()


def test_a_missing_token_inside_a_part_and_in_a_gap(eng, harness, tmp_path):
    from basevar_amd import _capi
    pf = [7, 207, 407]
    t, places = token_tile(pf, [3, 5])
    for s in (7, 206, 207, 406):  # first and last samples of both parts
        key = (t.beg + 1, s)
        short = ptm.Tile(t.chrom, t.beg, t.n, t.cell, t.qual, t.mapq, t.rank, {k: v for k, v in t.tokens.items() if k != key}, t.ref)
        assert ppm.run_parts(harness, tmp_path, short, pf) == ("missing",) + key
        for device in (False, True):
            eng.pileup_set_reference(t.ref)
            refused(eng, _capi.BV_ERR_DATA, "the indel cell at pos %d, sample %d has no token" % key, t.chrom, pf, tile=as_arg(short, device))
        same_as_model(eng, short, pf, first=0, n=1)  # the row before it is complete: the engine is usable
    for s in (6, 407):  # the edge samples of the gaps before and behind
        key = (t.beg + 1, s)
        short = ptm.Tile(t.chrom, t.beg, t.n, t.cell, t.qual, t.mapq, t.rank, {k: v for k, v in t.tokens.items() if k != key}, t.ref)
        same_as_model(eng, short, pf, harness, tmp_path)
        eng.pileup_set_reference(t.ref)
        with pytest.raises(RuntimeError, match="sample %d has no token" % s):  # the whole tile misses it
            eng.pileup_text(t.chrom, tile=as_arg(short))


# ------------------------------------------------------------------------------------------------------------------ 5. alignment
def test_chrom_of_1_to_40_bytes_and_the_alignment_census(eng):
    """every CHROM length 1 .. 40; and from the EXPECTED text: a part's start, a row's start, each of the five list starts and a
    tile boundary inside each list fall on all 16 residues modulo 16"""
    T = tile()
    pf = [3, 3 + T + 5, 3 + 2 * T + 14]
    t = ptm.random_tile(11, pf[-1] + 2, 3, 0.3, long_tokens=(2, 3, 63, 64, 65, 129, 200))
    part, line, lists, cuts = set(), set(), [set() for _ in range(5)], [set() for _ in range(5)]
    for ln in range(1, 41):
        t.chrom = (b"chromosome_with_a_long_name_0123456789_xyz")[:ln]
        text, off = same_as_model(eng, t, pf, device=ln % 2 == 0)
        for p in range(2):
            base = int(off[p * t.rows])
            if p:
                part.add(base % 16)
            places, total = ptm.row_places(ppm.slice_tile(t, pf[p], pf[p + 1]), T)
            assert base + total == int(off[(p + 1) * t.rows])
            for at, starts, cut in places:
                line.add((base + at) % 16)
                for l in range(5):
                    lists[l].add((base + starts[l]) % 16)
                    assert len(cut[l]) == 1
                    cuts[l].add((base + cut[l][0]) % 16)
    every = set(range(16))
    assert part == every and line == every and all(s == every for s in lists) and all(c == every for c in cuts)


# ---------------------------------------------------------------------------------------------------- 6. from a pileup (tile=None)
@pytest.fixture(scope="module")
def pileup_harness():
    return pr.build()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return pr.Corpus(tmp_path_factory.mktemp("pparts_corpus"), 65)


def pile(eng, d, window):
    return eng.pileup(d.records, d.run_off, d.run_sample, d.n_samples, d.tid, pr.REGION, window, pr.MAPQ_THD)


def test_parts_of_the_last_pileup_and_the_pileup_afterwards(eng, pileup_harness, corpus, tmp_path):
    """the BAM corpus piled up on the device: planes, tokens and token text are read where the pileup left them; pileup_rows and
    the submit work afterwards as before"""
    eng.pileup_set_reference(corpus.fa)
    for name in ("w65", "w1000", "edge"):
        window = pr.WINDOWS[name]
        d = pr.run_bam(pileup_harness, tmp_path / "d.bin", corpus, 65, window)[0]
        t = ptm.from_dump(d, pr.REF_ID, corpus.fa, window[0])
        pile(eng, d, window)
        before = submit_records(eng)
        for pf in ([0, 65], [0, 7, 14, 21, 28, 35, 42, 49, 56, 63, 65], [1, 9, 64]):
            off = eng.pileup_text_parts(pr.REF_ID, pf)
            want, want_off = ppm.parts_text(t, pf)
            assert (off == want_off).all() and fetch_between_sentinels(eng, int(off[-1])) == want, (name, pf)
        assert submit_records(eng) == before
        off = eng.pileup_text_parts(pr.REF_ID, [1, 9, 64], 3, 2)
        assert fetch_between_sentinels(eng, int(off[-1])) == ppm.parts_text(t, [1, 9, 64], 3, 2)[0]
        if name == "w1000":
            assert len(t.tokens) >= 4 and len(before[0]) > 0


# --------------------------------------------------------------------------------------------------------------------- 7. deflate
def block_table(lo, hi, block=0xff00):
    return list(range(lo, hi, block))


@pytest.mark.parametrize("level", ["fast", "small"])
def test_deflate_with_blocks_cut_at_part_boundaries(eng, level):
    """one deflate call whose block table is cut at the parts' starts: each part's members are bgzf_deflate's of that part's text"""
    t = ptm.random_tile(41, 300, 60, 0.08)
    pf = [0, 130, 137, 300]
    text, off = device_parts(eng, t, pf)
    starts = ppm.part_starts(off, 3)
    assert starts[1] - starts[0] > 0xff00 and starts[2] - starts[1] < 0xff00
    blocks, first_block = [], []
    for p in range(3):
        first_block.append(len(blocks))
        blocks += block_table(starts[p], starts[p + 1])
    first_block.append(len(blocks))
    members, member_off = eng.pileup_text_deflate(block_off=np.array(blocks + [starts[3]], np.uint64), level=level)
    assert member_off.size == len(blocks) + 1
    for p in range(3):
        part = text[starts[p]:starts[p + 1]]
        got = members[int(member_off[first_block[p]]):int(member_off[first_block[p + 1]])]
        want, want_off = eng.bgzf_deflate(part, level=level)
        assert got.tobytes() == want.tobytes() and (member_off[first_block[p]:first_block[p + 1] + 1] - member_off[first_block[p]] == want_off).all()
        assert inflate_members(got, want_off) == part == ppm.parts_text(t, pf[p:p + 2])[0]


# ------------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_engine_usable():
    import basevar_amd as bv
    from basevar_amd import _capi
    INV, BIG = _capi.BV_ERR_INVALID_ARG, _capi.BV_ERR_TOO_LARGE
    e = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(100), device=0, max_samples=256)
    t = ptm.random_tile(51, 70, 6, 0.6, beg=100)
    arg = as_arg(t)
    L = e._lib
    row_off = np.zeros(64, np.uint64)
    pf = np.array([0, 70], np.uint32)
    req = _capi.PileupText(None, b"c", 1, 0, 1, 0)
    parts = _capi.PileupTextParts(C.pointer(req), pf.ctypes.data, 1, 0)

    def call():
        return L.bv_engine_pileup_text_parts(e._h, C.byref(parts), row_off.ctypes.data, None), L.bv_last_error(e._h)

    assert L.bv_engine_pileup_text_parts(e._h, None, row_off.ctypes.data, None) == INV and b"null in/rows/row_off" in L.bv_last_error(e._h)
    assert L.bv_engine_pileup_text_parts(e._h, C.byref(parts), None, None) == INV and b"null in/rows/row_off" in L.bv_last_error(e._h)
    parts.rows = None
    assert call()[0] == INV and b"null in/rows/row_off" in call()[1]
    parts.rows = C.pointer(req)
    parts.reserved_ = 1
    assert call()[0] == INV and b"reserved_ must be zero" in call()[1]
    parts.reserved_ = 0
    parts.part_first = None
    assert call()[0] == INV and b"at least one part" in call()[1]
    parts.part_first, parts.n_parts = pf.ctypes.data, 0
    assert call()[0] == INV and b"at least one part" in call()[1]
    parts.n_parts = 1
    req.reserved_ = 1
    assert call()[0] == INV and b"reserved_ must be zero" in call()[1]
    req.reserved_ = 0
    assert (row_off == 0).all()
    # bv_engine_pileup_text's own refusals come through
    refused(e, INV, "no reference set", "c", [0, 70], tile=arg)
    e.pileup_set_reference(t.ref)
    refused(e, INV, "no completed bv_engine_pileup", "c", [0, 70])
    refused(e, INV, "chrom must have 1 to 255 bytes", b"", [0, 70], tile=arg)
    refused(e, INV, "are beyond the tile's 6", "c", [0, 70], 0, 7, tile=arg)
    bad = dict(arg, pitch=t.pitch + 8)
    refused(e, INV, "pitch must be", "c", [0, 70], tile=bad)
    # the part table
    refused(e, INV, "part 0 is empty or descends", "c", [5, 5], tile=arg)
    refused(e, INV, "part 1 is empty or descends", "c", [0, 10, 10, 70], tile=arg)
    refused(e, INV, "part 1 is empty or descends", "c", [0, 10, 9, 70], tile=arg)
    refused(e, INV, "the parts end at sample 71, beyond the tile's 70", "c", [0, 71], tile=arg)
    refused(e, INV, "at least one part", "c", [3], tile=arg)
    refused(e, INV, "at least one part", "c", [], tile=arg)
    # too many workgroups: rows x the tiles of all parts (a tile that claims 2^20 rows of 64 tiles: refused before anything is read)
    T = tile()
    wide = dict(arg, rows=1 << 20, n_samples=64 * T, pitch=64 * T)
    e.pileup_set_reference(b"A" * ((1 << 20) + 200))
    refused(e, BIG, "reaches 2^26", "c", [0, 32 * T, 64 * T], 0, 1 << 20, tile=wide)
    assert e.pileup_text_parts("c", [0, 32 * T, 63 * T + 1], 0, 0, tile=wide).tolist() == [0]
    e.pileup_set_reference(t.ref)
    # ... and the engine still formats
    text, off = device_parts(e, t, [0, 30, 70], arg=arg)
    assert text == ppm.parts_text(t, [0, 30, 70])[0]
    # n = 0: an empty text
    assert e.pileup_text_parts("c", [0, 30, 70], 3, 0, tile=arg).tolist() == [0] and e.pileup_text_fetch().size == 0
    e.close()
