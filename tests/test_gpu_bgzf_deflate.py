"""GPU tests of bv_engine_bgzf_deflate (include/basevar_amd_bgzf.h): the corpus of tests/deflate_corpus.py deflated on the
device.  The oracle is the CPU build of the same encoder core (tests/test_deflate_cpu.py holds it to zlib, to the device
decoder's core and to the size condition under ASan + UBSan): the device's members are its members, byte for byte.  Over the
edge corpus (deflate_corpus.edge_corpus()) the oracle is tests/deflate_model.py, a serial restatement of the encoder's definition
that shares no code with the kernel, and the CPU build beside it."""
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
import deflate_model as dm  # noqa: E402


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """[(name, text, sizes, the CPU core's members back to back)]"""
    d = tmp_path_factory.mktemp("deflate_gpu")
    emit = dc.cxx("emit_corpus", d)
    core = dc.cxx("deflate_core_check", d)
    return [(name, text, sizes, dc.cpu_members(core, text, sizes, d)) for name, text, sizes in dc.corpus(emit)]


@pytest.fixture()
def eng():
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(20000), device=0)
    yield e
    e.close()


def joined(corpus):
    """the whole corpus as one text and one list of blocks"""
    text = b"".join(t for _, t, _, _ in corpus)
    sizes = [s for _, _, ss, _ in corpus for s in ss]
    return text, sizes, b"".join(m for _, _, _, m in corpus)


def test_device_members_are_the_cpu_cores_bytes(eng, corpus):
    for name, text, sizes, expect in corpus:
        members, off = eng.bgzf_deflate(text, block_off=dc.offsets(sizes))
        assert off[0] == 0 and len(off) == len(sizes) + 1 and int(off[-1]) == members.size, name
        assert members.tobytes() == expect, name
        cut = dc.split_members(members.tobytes())
        assert [len(m) for m in cut] == [int(b - a) for a, b in zip(off[:-1], off[1:])], name
        for m, block in zip(cut, dc.blocks_of(text, sizes)):
            dc.check_member(m, block)


def test_size_of_the_device_members_of_vcf_records_against_zlib(eng, corpus):
    """the condition on the size, on what the device wrote: at most 2.5 times zlib's level 6 for the same blocks"""
    name, text, sizes, _ = corpus[0]
    assert name == "vcf"
    members, off = eng.bgzf_deflate(text)  # (the default cut: 0xff00)
    assert len(off) - 1 == len(sizes)
    l6 = sum(dc.zlib_member_bytes(b, 6) for b in dc.blocks_of(text, sizes))
    print("vcf: %d bytes of text, %d in the device's members, zlib level 6 %d (x %.3f)" % (len(text), members.size, l6, members.size / l6))
    assert members.size <= 2.5 * l6


def test_text_given_as_a_device_pointer(eng, corpus):
    import torch
    text, sizes, expect = joined(corpus)
    # (behind 3 bytes: the text then starts off every aligned word)
    dev = torch.zeros(3 + len(text), dtype=torch.uint8, device="cuda:0")
    dev[3:] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    members, off = eng.bgzf_deflate(dev[3:], block_off=dc.offsets(sizes))
    assert members.tobytes() == expect
    host, off_h = eng.bgzf_deflate(text, block_off=dc.offsets(sizes))
    assert host.tobytes() == expect and (off == off_h).all()


def test_the_file_reads_back_with_gzip_and_with_the_device_inflate(eng, corpus, tmp_path):
    from basevar_amd import _capi
    text, sizes, _ = joined(corpus)
    members, off = eng.bgzf_deflate(text, block_off=dc.offsets(sizes))
    path = tmp_path / "out.gz"
    path.write_bytes(members.tobytes() + dc.EOF_MARKER)
    with gzip.open(path, "rb") as fh:
        assert fh.read() == text
    back, dst_off, status = eng.bgzf_inflate(members, off)
    assert (status == _capi.BV_BGZF_OK).all() and back.tobytes() == text
    assert [int(b - a) for a, b in zip(dst_off[:-1], dst_off[1:])] == sizes


def test_a_call_that_crosses_staging_chunks(eng, corpus, monkeypatch):
    """five blocks a chunk: the two slots of the staging are reused many times, the last chunk is short"""
    text, sizes, expect = joined(corpus)
    assert len(sizes) > 5 * 2 * 3 and len(sizes) % 5
    monkeypatch.setenv("BASEVAR_AMD_DEFLATE_CHUNK_BLOCKS", "5")
    members, off = eng.bgzf_deflate(text, block_off=dc.offsets(sizes))
    assert members.tobytes() == expect
    monkeypatch.setenv("BASEVAR_AMD_DEFLATE_CHUNK_BLOCKS", "1")
    members, off = eng.bgzf_deflate(text[:400000])
    monkeypatch.delenv("BASEVAR_AMD_DEFLATE_CHUNK_BLOCKS")
    again, off2 = eng.bgzf_deflate(text[:400000])
    assert members.tobytes() == again.tobytes() and (off == off2).all()


def test_blocks_that_do_not_cover_the_text(eng, corpus):
    """the first block need not start the text, the last need not end it: what lies outside is not coded"""
    name, text, _, _ = corpus[0]
    off = np.array([5, 70000, 70001, 70001 + 0xff00], np.uint64)
    off[1] = 5 + 0xff00 - 3
    off[2:] = off[1] + np.array([1, 1 + 0xff00], np.uint64)
    members, moff = eng.bgzf_deflate(text, block_off=off)
    cut = dc.split_members(members.tobytes())
    assert len(cut) == 3 and int(moff[3]) == members.size
    for m, (a, b) in zip(cut, zip(off[:-1], off[1:])):
        dc.check_member(m, text[int(a):int(b)])


def raw_call(eng, text, off, n=None, kind=None, dst="room", cap=None, moff="room", text_bytes=None, null_text=False, null_off=False):
    from basevar_amd import _capi
    buf = np.frombuffer(text, np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    n = len(off) - 1 if n is None else n
    room = np.full(len(text) + 31 * max(n, 1) + 64, 0xA5, np.uint8)
    member_off = np.full(n + 2, 0xEEEE, np.uint64)
    rc = eng._lib.bv_engine_bgzf_deflate(eng._h, None if null_text else buf.ctypes.data, len(text) if text_bytes is None else text_bytes,
                                         _capi.BV_MEM_HOST if kind is None else kind, None if null_off else off.ctypes.data, n,
                                         room.ctypes.data if dst == "room" else None, len(text) + 31 * n if cap is None else cap,
                                         member_off.ctypes.data if moff == "room" else None, None)
    return rc, room, member_off


def test_every_refusal(eng, corpus):
    from basevar_amd import _capi
    bad = _capi.BV_ERR_INVALID_ARG
    text = corpus[0][1][:200000]
    good = np.array([0, 0xff00, 2 * 0xff00, 3 * 0xff00, 200000], np.uint64)
    rc, room, moff = raw_call(eng, text, good)
    assert rc == 0 and moff[0] == 0 and (room[int(moff[4]):] == 0xA5).all()
    full = room[:int(moff[4])].tobytes()
    for what, kw in (("null text", dict(null_text=True)), ("null block_off", dict(null_off=True)), ("null dst", dict(dst=None)),
                     ("null member_off", dict(moff=None)), ("a bad memory kind", dict(kind=7)), ("a negative memory kind", dict(kind=-1)),
                     ("one byte short of the worst case", dict(cap=200000 + 31 * 4 - 1)), ("text_bytes before the last offset", dict(text_bytes=199999))):
        rc, room, moff = raw_call(eng, text, good, **kw)
        assert rc == bad, what
        assert (room == 0xA5).all(), what
        assert eng._err(), what
    for what, off in (("an empty block", [0, 0xff00, 0xff00, 3 * 0xff00 - 5, 200000]), ("a block of 0xff01 bytes", [0, 0xff01, 2 * 0xff00, 3 * 0xff00, 200000]),
                      ("offsets out of order", [0, 0xff00, 0xfe00, 3 * 0xfe00, 200000]), ("an offset beyond the text", [0, 0xff00, 2 * 0xff00, 3 * 0xff00, 200001]),
                      ("a first block that is empty", [7, 7, 100, 200])):
        rc, room, moff = raw_call(eng, text, np.array(off, np.uint64))
        assert rc == bad and (room == 0xA5).all(), what
    assert eng._lib.bv_engine_bgzf_deflate(None, None, 0, _capi.BV_MEM_HOST, None, 0, None, 0, None, None) == bad
    # the worst case itself is room enough, and the engine works after the refusals
    rc, room, moff = raw_call(eng, text, good, cap=200000 + 31 * 4)
    assert rc == 0 and room[:int(moff[4])].tobytes() == full


def test_no_blocks(eng):
    from basevar_amd import _capi
    rc, room, moff = raw_call(eng, b"xyz", np.array([0], np.uint64), n=0)
    assert rc == 0 and moff[0] == 0 and moff[1] == 0xEEEE and (room == 0xA5).all()
    # nothing but member_off is looked at
    moff = np.full(2, 0xEEEE, np.uint64)
    assert eng._lib.bv_engine_bgzf_deflate(eng._h, None, 0, _capi.BV_MEM_HOST, None, 0, None, 0, moff.ctypes.data, None) == 0
    assert moff[0] == 0 and moff[1] == 0xEEEE
    members, off = eng.bgzf_deflate(b"")
    assert members.size == 0 and off.tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------------------
# the device against the model (tests/deflate_model.py) over the edge corpus

_model = {}


def model_member(block):
    if block not in _model:
        _model[block] = dm.member(block)
    return _model[block]


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    """([(name, [blocks])], text, sizes, the model's members back to back, the CPU core's)"""
    d = tmp_path_factory.mktemp("deflate_edge_gpu")
    core = dc.cxx("deflate_core_check", d)
    entries = dc.edge_corpus()
    text, sizes = dc.edge_text(entries)
    model = b"".join(model_member(b) for b in dc.blocks_of(text, sizes))
    return entries, text, sizes, model, dc.cpu_members(core, text, sizes, d)


def test_edge_members_are_the_models_bytes_and_the_cpu_cores(eng, edge):
    _, text, sizes, model, cpu = edge
    members, off = eng.bgzf_deflate(text, block_off=dc.offsets(sizes))
    dc.assert_members(members.tobytes(), model, sizes, "the device against the model")
    dc.assert_members(members.tobytes(), cpu, sizes, "the device against the CPU build")
    assert off.tolist() == dc.offsets([len(m) for m in dc.split_members(model)]).tolist()


def test_edge_text_as_a_device_pointer_at_every_misalignment(eng, edge):
    """The slices [0:], [1:], [2:], [3:] of one allocation of len(text) + 3 bytes, each filled to its end: the text, and a last
    block of the 3, 2, 1 or 0 bytes that are left, so that the last block ends with the slice whatever its base."""
    import torch
    _, text, sizes, model, _ = edge
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
        members, off = eng.bgzf_deflate(view, block_off=dc.offsets(ss))
        dc.assert_members(members.tobytes(), model + (model_member(rest) if rest else b""), ss, "a text %d bytes behind an aligned word" % k)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 2500])
def test_member_off_is_the_running_sum_of_the_models_sizes(eng, edge, monkeypatch, n):
    """n small blocks in one call with the staging as it is: the 256 threads of the scan have no block, one, or several, and
    calls of more than 1024 blocks cross staging chunks by themselves"""
    monkeypatch.delenv("BASEVAR_AMD_DEFLATE_CHUNK_BLOCKS", raising=False)
    entries = dict(edge[0])
    pool = [b for b in entries["ends"] + entries["collisions"] + entries["stored_or_fixed"] if len(b) < 200]
    assert len(pool) > 150 and {len(b) for b in pool} >= set(range(1, 8))
    blocks = [pool[(k * 37 + k // len(pool)) % len(pool)] for k in range(n)]
    expect = [model_member(b) for b in blocks]
    assert n < 200 or len({len(m) for m in expect}) > 40
    members, off = eng.bgzf_deflate(b"".join(blocks), block_off=dc.offsets([len(b) for b in blocks]))
    assert off.dtype == np.uint64 and off.tolist() == dc.offsets([len(m) for m in expect]).tolist()
    dc.assert_members(members.tobytes(), b"".join(expect), [len(b) for b in blocks], "%d small blocks" % n)


def test_edge_members_do_not_depend_on_the_staging_chunk(eng, edge, monkeypatch):
    _, text, sizes, model, _ = edge
    monkeypatch.setenv("BASEVAR_AMD_DEFLATE_CHUNK_BLOCKS", "3")
    members, off = eng.bgzf_deflate(text, block_off=dc.offsets(sizes))
    dc.assert_members(members.tobytes(), model, sizes, "three blocks a staging chunk")
    assert int(off[-1]) == len(model)


def test_the_device_inflate_reads_the_edge_members_back(eng, edge):
    from basevar_amd import _capi
    _, text, sizes, model, _ = edge
    members, off = eng.bgzf_deflate(text, block_off=dc.offsets(sizes))
    back, dst_off, status = eng.bgzf_inflate(members, off)
    assert (status == _capi.BV_BGZF_OK).all() and back.tobytes() == text
    assert [int(b - a) for a, b in zip(dst_off[:-1], dst_off[1:])] == sizes
