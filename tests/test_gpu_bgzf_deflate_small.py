"""GPU tests of bv_engine_bgzf_deflate_level at BV_DEFLATE_SMALL (include/basevar_amd_bgzf.h): the corpus and the edge corpus of
tests/deflate_corpus.py and the blocks of tests/deflate_small_corpus.py deflated on the device.  The device's members are,
byte for byte, those of the CPU build of the same core (tests/cpp/deflate_core_check.cpp --level small; tests/test_deflate_small_cpu.py
runs it under ASan + UBSan) and those of tests/deflate_small_model.py, a serial restatement of the level's definition that shares
no code with the kernel.

No text was found that drives a code past 15 bits (tests/test_deflate_small_cpu.py says why): the depth limit is covered on
the device by the count vectors of deflate_small_corpus.count_vectors() through bv_engine_deflate_code_lengths."""
import ctypes as C
import gzip
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_corpus as dc  # noqa: E402
import deflate_small_corpus as sc  # noqa: E402
import deflate_small_model as sm  # noqa: E402


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """[(name, text, sizes, the model's members back to back, the CPU core's)]: corpus(), and both edge corpora as one entry"""
    d = tmp_path_factory.mktemp("deflate_small_gpu")
    emit = dc.cxx("emit_corpus", d)
    core = dc.cxx("deflate_core_check", d)
    entries = list(dc.corpus(emit))
    edge = dc.edge_corpus() + sc.small_edge_corpus(emit)
    text, sizes = dc.edge_text(edge)
    entries.append(("edge", text, sizes))
    return [(name, text, sizes, b"".join(sm.member(b) for b in dc.blocks_of(text, sizes)), dc.cpu_members(core, text, sizes, d, level="small")) for name, text, sizes in entries]


@pytest.fixture()
def eng():
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(20000), device=0)
    yield e
    e.close()


def test_device_members_are_the_models_bytes_and_the_cpu_cores(eng, corpus):
    for name, text, sizes, model, cpu in corpus:
        members, off = eng.bgzf_deflate(text, block_off=dc.offsets(sizes), level="small")
        assert off[0] == 0 and len(off) == len(sizes) + 1 and int(off[-1]) == members.size, name
        dc.assert_members(members.tobytes(), model, sizes, name + ": the device against the model")
        dc.assert_members(members.tobytes(), cpu, sizes, name + ": the device against the CPU build")
        assert off.tolist() == dc.offsets([len(m) for m in dc.split_members(model)]).tolist(), name


def test_size_of_the_device_members_against_zlib_and_the_fast_level(eng, corpus):
    """the cap of tests/test_deflate_small_cpu.py on what the device wrote: VCF, CVG and batchfile text at most 1.15 times zlib's
    level 6, every entry at most the fast level's members plus 4 bytes a block"""
    for name, text, sizes, _, _ in corpus[:-1]:
        off = dc.offsets(sizes)
        small, _ = eng.bgzf_deflate(text, block_off=off, level="small")
        fast, _ = eng.bgzf_deflate(text, block_off=off, level="fast")
        l6 = sum(dc.zlib_member_bytes(b, 6) for b in dc.blocks_of(text, sizes))
        print("%s: %d bytes of text, small %d (x %.3f of zlib level 6's %d), fast %d" % (name, len(text), small.size, small.size / l6, l6, fast.size))
        if name in ("vcf", "cvg", "rows"):
            assert small.size <= 1.15 * l6, name
        assert small.size <= fast.size + 4 * len(sizes), name
    assert [c[0] for c in corpus[:3]] == ["vcf", "cvg", "rows"]


def test_edge_text_as_a_device_pointer_at_every_misalignment(eng, corpus):
    """The slices [0:], [1:], [2:], [3:] of one allocation of len(text) + 3 bytes, each filled to its end: the text, and a last
    block of the 3, 2, 1 or 0 bytes that are left, so that the last block ends with the slice whatever its base."""
    import torch
    _, text, sizes, model, _ = corpus[-1]
    assert {s % 4 for s in sizes} == {0, 1, 2, 3}
    buf = torch.zeros(len(text) + 3, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 4 == 0
    for k in range(4):
        rest = text[:3 - k]
        fill, ss = text + rest, sizes + ([len(rest)] if rest else [])
        buf[k:] = torch.frombuffer(bytearray(fill), dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        view = buf[k:]
        assert view.data_ptr() % 4 == k and view.numel() == sum(ss)
        members, off = eng.bgzf_deflate(view, block_off=dc.offsets(ss), level="small")
        dc.assert_members(members.tobytes(), model + (sm.member(rest) if rest else b""), ss, "a text %d bytes behind an aligned word" % k)


def test_members_do_not_depend_on_the_staging_chunk(eng, corpus, monkeypatch):
    _, text, sizes, model, _ = corpus[-1]
    monkeypatch.setenv("BASEVAR_AMD_DEFLATE_CHUNK_BLOCKS", "3")
    members, off = eng.bgzf_deflate(text, block_off=dc.offsets(sizes), level="small")
    dc.assert_members(members.tobytes(), model, sizes, "three blocks a staging chunk")
    assert int(off[-1]) == len(model)


def test_1025_small_blocks_in_one_call(eng, corpus, monkeypatch):
    """more blocks than a staging chunk holds, every one with a token run of its own"""
    monkeypatch.delenv("BASEVAR_AMD_DEFLATE_CHUNK_BLOCKS", raising=False)
    _, text, sizes, model, _ = corpus[-1]
    pool = [(b, m) for b, m in zip(dc.blocks_of(text, sizes), dc.split_members(model)) if len(b) < 400]
    assert len(pool) > 300 and {m[18] >> 1 & 3 for _, m in pool} == {0, 1, 2}
    picked = [pool[(k * 37 + k // len(pool)) % len(pool)] for k in range(1025)]
    blocks, expect = [b for b, _ in picked], [m for _, m in picked]
    members, off = eng.bgzf_deflate(b"".join(blocks), block_off=dc.offsets([len(b) for b in blocks]), level="small")
    assert off.tolist() == dc.offsets([len(m) for m in expect]).tolist()
    dc.assert_members(members.tobytes(), b"".join(expect), [len(b) for b in blocks], "1025 small blocks")


def raw_call(eng, text, off, level, entry="bv_engine_bgzf_deflate_level"):
    from basevar_amd import _capi
    buf = np.frombuffer(text, np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    n = len(off) - 1
    room = np.full(len(text) + 31 * n + 64, 0xA5, np.uint8)
    member_off = np.full(n + 2, 0xEEEE, np.uint64)
    if entry == "bv_engine_bgzf_deflate":
        rc = eng._lib.bv_engine_bgzf_deflate(eng._h, buf.ctypes.data, len(text), _capi.BV_MEM_HOST, off.ctypes.data, n, room.ctypes.data, len(text) + 31 * n,
                                             member_off.ctypes.data, None)
    else:
        rc = eng._lib.bv_engine_bgzf_deflate_level(eng._h, buf.ctypes.data, len(text), _capi.BV_MEM_HOST, off.ctypes.data, n, level, room.ctypes.data,
                                                   len(text) + 31 * n, member_off.ctypes.data, None)
    return rc, room, member_off


def test_level_0_is_the_old_entry_point_and_a_bad_level_is_refused(eng, corpus):
    from basevar_amd import _capi
    assert (_capi.BV_DEFLATE_FAST, _capi.BV_DEFLATE_SMALL) == (0, 1)
    text = corpus[0][1][:200000]
    off = np.array([0, 0xff00, 2 * 0xff00, 3 * 0xff00, 200000], np.uint64)
    rc, old, old_off = raw_call(eng, text, off, None, entry="bv_engine_bgzf_deflate")
    assert rc == 0
    rc, new, new_off = raw_call(eng, text, off, _capi.BV_DEFLATE_FAST)
    assert rc == 0 and (old == new).all() and (old_off == new_off).all()
    rc, small, small_off = raw_call(eng, text, off, _capi.BV_DEFLATE_SMALL)
    assert rc == 0 and small_off[4] < new_off[4] and (small[int(small_off[4]):] == 0xA5).all()
    for level in (2, -1, 6, 1 << 20):
        rc, room, moff = raw_call(eng, text, off, level)
        assert rc == _capi.BV_ERR_INVALID_ARG and (room == 0xA5).all() and (moff == 0xEEEE).all() and b"level" in eng._err().encode(), level
    with pytest.raises(ValueError):
        eng.bgzf_deflate(text, level="best")
    # the refusals of the old entry point hold at the new level, and the engine works after them
    rc, room, moff = raw_call(eng, text, np.array([0, 0xff01, 200000], np.uint64), _capi.BV_DEFLATE_SMALL)
    assert rc == _capi.BV_ERR_INVALID_ARG and (room == 0xA5).all()
    rc, again, again_off = raw_call(eng, text, off, _capi.BV_DEFLATE_SMALL)
    assert rc == 0 and (again == small).all() and (again_off == small_off).all()
    members, moff = eng.bgzf_deflate(b"", level="small")
    assert members.size == 0 and moff.tolist() == [0]


def test_the_file_reads_back_with_gzip_and_with_the_device_inflate(eng, corpus, tmp_path):
    from basevar_amd import _capi
    text = b"".join(t for _, t, _, _, _ in corpus)
    sizes = [s for _, _, ss, _, _ in corpus for s in ss]
    members, off = eng.bgzf_deflate(text, block_off=dc.offsets(sizes), level="small")
    path = tmp_path / "out.gz"
    path.write_bytes(members.tobytes() + dc.EOF_MARKER)
    with gzip.open(path, "rb") as fh:
        assert fh.read() == text
    back, dst_off, status = eng.bgzf_inflate(members, off)
    assert (status == _capi.BV_BGZF_OK).all() and back.tobytes() == text
    assert [int(b - a) for a, b in zip(dst_off[:-1], dst_off[1:])] == sizes


def test_code_lengths_of_count_vectors_on_the_device(eng):
    """the depth limit on the device: the lengths and the rounds of halving are the model's, for every count vector"""
    from basevar_amd import _capi
    rounds_seen, named_rounds = {}, {}
    for name, limit, counts in sc.count_vectors():
        lengths, rounds = eng.deflate_code_lengths(counts, limit)
        want = sm.code_lengths(counts, limit)
        assert (lengths.tolist(), rounds) == want, name
        assert sc.kraft_is_one(lengths.tolist()) and int(lengths.max()) <= limit, name
        rounds_seen.setdefault((len(counts), limit), set()).add(rounds)
        named_rounds[name] = rounds
    for key in ((286, 15), (30, 15), (19, 7)):
        assert {0, 1, 2} <= rounds_seen[key], (key, rounds_seen[key])
    # the Fibonacci vectors of one and of two rounds, by name
    assert {name: r for name, r in named_rounds.items() if name in sc.FIBONACCI_ROUNDS} == sc.FIBONACCI_ROUNDS
    out, r = np.zeros(300, np.uint8), C.c_uint32(77)
    for n, limit, counts in ((1, 15, [1]), (287, 15, [1] * 287), (19, 4, [1] * 19), (30, 0, [1] * 30), (30, 16, [1] * 30), (2, 15, [1 << 31, 1 << 31])):
        c = np.array(counts, np.uint32)
        assert eng._lib.bv_engine_deflate_code_lengths(eng._h, c.ctypes.data, n, limit, out.ctypes.data, C.byref(r), None) == _capi.BV_ERR_INVALID_ARG
    assert not out.any() and r.value == 77
