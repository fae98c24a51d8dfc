"""GPU tests of bv_engine_bgzf_inflate (include/basevar_amd_bgzf.h): the corpus of tests/bgzf_corpus.py inflated on the device
against zlib, and the damaged corpus against the verdicts of the decoder core's CPU build (which tests/test_bgzf_cpu.py holds
to zlib under ASan + UBSan)."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzf_corpus as bc  # noqa: E402

GUARD = 67  # (odd on purpose: the text then starts off every 16-byte line of the destination)


@pytest.fixture(scope="module")
def valid():
    return bc.valid_corpus()


@pytest.fixture()
def eng():
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(20000), device=0)
    yield e
    e.close()


def raw_inflate(eng, members, device, capacity_slack=0, dst=None):
    """bv_engine_bgzf_inflate into a buffer with guard bytes on both sides: (rc, text incl. guards, dst_off, status); dst: a
    device tensor of 0xA5 bytes to use (at least the guards and the text)"""
    import torch
    from basevar_amd import _capi
    data, off = bc.pack(members)
    buf = np.frombuffer(data, np.uint8)
    n = len(members)
    dst_off = np.zeros(n + 1, np.uint64)
    status = np.full(n, 0xEE, np.uint8)
    mb = _capi.BgzfMembers(buf.ctypes.data, off.ctypes.data, int(buf.size), n, 0)
    # the size first: a call without room writes dst_off and refuses
    rc = eng._lib.bv_engine_bgzf_inflate(eng._h, C.byref(mb), None, 0, _capi.BV_MEM_HOST, dst_off.ctypes.data, status.ctypes.data, None)
    total = int(dst_off[n])
    assert rc == (_capi.BV_ERR_INVALID_ARG if total else 0)
    if dst is not None:
        assert device and dst.numel() >= GUARD + total + GUARD + capacity_slack
        ptr = dst.data_ptr() + GUARD
    elif device:
        dst = torch.full((GUARD + total + GUARD + capacity_slack,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ptr = dst.data_ptr() + GUARD
    else:
        dst = np.full(GUARD + total + GUARD + capacity_slack, 0xA5, np.uint8)
        ptr = dst.ctypes.data + GUARD
    rc = eng._lib.bv_engine_bgzf_inflate(eng._h, C.byref(mb), ptr, total + capacity_slack, _capi.BV_MEM_DEVICE if device else _capi.BV_MEM_HOST,
                                         dst_off.ctypes.data, status.ctypes.data, None)
    text = dst.cpu().numpy() if device else dst
    return rc, text, dst_off, status


def check_valid(text, dst_off, status, datas):
    assert (status == 0).all(), np.nonzero(status)[0][:10]
    assert np.array_equal(dst_off, np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.uint64))
    assert text[GUARD:GUARD + int(dst_off[-1])].tobytes() == b"".join(datas)
    assert (text[:GUARD] == 0xA5).all() and (text[GUARD + int(dst_off[-1]):] == 0xA5).all()


@pytest.mark.parametrize("device", [False, True], ids=["host_dst", "device_dst"])
def test_whole_valid_corpus_in_one_call(eng, valid, device):
    members = [m for _, m, _ in valid]
    datas = [d for _, _, d in valid]
    for m, d in zip(members, datas):
        assert zlib.decompress(bc.payload_of(m), -15) == d  # the oracle: zlib
    rc, text, dst_off, status = raw_inflate(eng, members, device)
    assert rc == 0, eng._err()
    check_valid(text, dst_off, status, datas)


def test_valid_corpus_one_member_per_call(eng, valid):
    for name, m, d in valid:
        text, dst_off, status = eng.bgzf_inflate(m, [0, len(m)])
        assert status.tolist() == [0] and dst_off.tolist() == [0, len(d)] and text.tobytes() == d, name


def test_no_member_and_only_the_end_marker(eng):
    text, dst_off, status = eng.bgzf_inflate(b"", [0])
    assert text.size == 0 and dst_off.tolist() == [0] and status.size == 0
    eof = bc.member(b"")
    assert len(eof) == 28
    text, dst_off, status = eng.bgzf_inflate(eof * 3, [0, 28, 56, 84])
    assert text.size == 0 and dst_off.tolist() == [0, 0, 0, 0] and status.tolist() == [0, 0, 0]


@pytest.mark.parametrize("device", [False, True], ids=["host_dst", "device_dst"])
def test_staging_reused_over_many_chunks(eng, valid, device, monkeypatch):
    """a chunk of 100 000 compressed bytes: the corpus, three times over, crosses both staging slots many times"""
    monkeypatch.setenv("BASEVAR_AMD_TEXT_CHUNK_BYTES", "100000")
    members = [m for _, m, _ in valid] * 3
    datas = [d for _, _, d in valid] * 3
    assert sum(len(m) for m in members) > 20 * 100000
    rc, text, dst_off, status = raw_inflate(eng, members, device)
    assert rc == 0, eng._err()
    check_valid(text, dst_off, status, datas)


def test_more_than_128_mib_of_text(eng):
    """2 400 members of 64 KiB of rows each, level 1 and 6 by turns: 150 MiB of text in one call, default chunks"""
    a, b = bc.rows_text(65536, seed=21), bc.rows_text(65536, seed=22)
    pool = [(bc.member(a, 1), a), (bc.member(b, 6), b), (bc.member(a[:65000], 0), a[:65000])]
    members = [pool[k % 3][0] for k in range(2400)]
    text, dst_off, status = eng.bgzf_inflate(b"".join(members), np.concatenate([[0], np.cumsum([len(m) for m in members])]))
    assert (status == 0).all() and int(dst_off[-1]) > (128 << 20)
    for k in (0, 1, 2, 1198, 2397, 2398, 2399):
        assert text[int(dst_off[k]):int(dst_off[k + 1])].tobytes() == pool[k % 3][1], k
    # every member, by its CRC32
    for k in range(2400):
        assert zlib.crc32(text[int(dst_off[k]):int(dst_off[k + 1])]) == zlib.crc32(pool[k % 3][1]), k


@pytest.mark.parametrize("device", [False, True], ids=["host_dst", "device_dst"])
def test_damaged_members_between_valid_ones(eng, valid, device, tmp_path):
    """Reporting: every damaged member gets the status the CPU build of the core gives it, its valid neighbours' bytes and the
    guard bytes around dst are intact, the call returns BV_OK and the engine goes on serving lrt()."""
    import basevar_amd as bv
    from basevar_amd.synth import make_slab
    damaged = bc.damaged_corpus()
    p, rows = bc.core_verdicts(bc.build_core_check(tmp_path), [m for _, m in damaged], tmp_path)
    assert p.returncode == 0 and len(rows) == len(damaged), p.stderr[-2000:]
    good = [(m, d) for _, m, d in valid if len(d) > 0][:40]
    members, expect, datas = [], [], []
    for k, ((name, m), r) in enumerate(zip(damaged, rows)):
        g = good[k % len(good)]
        members += [g[0], m]
        expect += [0, r[0]]
        datas += [g[1], None]
    members.append(good[0][0]); expect.append(0); datas.append(good[0][1])
    slab = make_slab(48, 20000, seed=5, coverage=0.08, n_groups=2)
    fresh = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(20000), device=0)
    try:
        exp = fresh.lrt(slab)
    finally:
        fresh.close()
    rc, text, dst_off, status = raw_inflate(eng, members, device)
    assert rc == 0, eng._err()
    wrong = [(k, damaged[k // 2][0] if k % 2 else "valid", int(status[k]), e) for k, e in enumerate(expect) if status[k] != e]
    assert not wrong, wrong[:20]
    assert len(set(status.tolist())) == 5
    for k, d in enumerate(datas):
        lo, hi = int(dst_off[k]), int(dst_off[k + 1])
        if d is not None:
            assert text[GUARD + lo:GUARD + hi].tobytes() == d, k
        elif status[k] == 0:  # damaged, and valid all the same: zlib's bytes
            assert text[GUARD + lo:GUARD + hi].tobytes() == zlib.decompress(bc.payload_of(members[k]), -15), k
    assert (text[:GUARD] == 0xA5).all() and (text[GUARD + int(dst_off[-1]):] == 0xA5).all()
    got = eng.lrt(slab)
    assert got.sites.tobytes() == exp.sites.tobytes() and got.groups.tobytes() == exp.groups.tobytes()
    assert got.n_variant == exp.n_variant and exp.n_variant > 0


def test_argument_errors(eng, valid):
    from basevar_amd import _capi
    m = valid[0][1]
    buf = np.frombuffer(m + m, np.uint8)
    dst = np.zeros(1 << 18, np.uint8)
    dst_off = np.zeros(3, np.uint64)
    status = np.zeros(2, np.uint8)

    def call(off, data_bytes=None, cap=dst.size, kind=_capi.BV_MEM_HOST, reserved=0, dstp=dst.ctypes.data, offp=dst_off.ctypes.data, stp=status.ctypes.data):
        o = np.asarray(off, np.uint64)
        mb = _capi.BgzfMembers(buf.ctypes.data, o.ctypes.data, buf.size if data_bytes is None else data_bytes, o.size - 1, reserved)
        return eng._lib.bv_engine_bgzf_inflate(eng._h, C.byref(mb), dstp, cap, kind, offp, stp, None)
    L = len(m)
    assert call([0, L, 2 * L]) == 0 and status.tolist() == [0, 0]
    for rc in (call([0, L, 2 * L], offp=None), call([0, L, 2 * L], stp=None), call([0, L, 2 * L], dstp=None), call([L, 0, 2 * L]),
               call([0, L, 2 * L + 1]), call([0, L, 2 * L], data_bytes=2 * L - 1), call([0, 25, 2 * L]), call([0, L, 2 * L], cap=2 * len(valid[0][2]) - 1),
               call([0, L, 2 * L], kind=7), call([0, L, 2 * L], reserved=1)):
        assert rc == _capi.BV_ERR_INVALID_ARG
        assert b"bv_engine_bgzf_inflate" in eng._lib.bv_last_error(eng._h)
    assert call([0, L, 2 * L]) == 0 and status.tolist() == [0, 0]
    # a member cut short in the packing: the BC field no longer agrees -> a status, not an argument error
    assert call([0, L - 1, 2 * L]) == 0 and status[0] == _capi.BV_BGZF_BAD_HEADER


# ---- members that zlib's compressor never writes (bc.foreign_corpus(), made with tests/deflate_writer.py; zlib is the judge)


@pytest.fixture(scope="module")
def foreign():
    out = bc.foreign_corpus()
    for _, m, d in out:
        xlen = int.from_bytes(m[10:12], "little")
        assert zlib.decompress(m[12 + xlen:-8], -15) == d  # the oracle: zlib
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host_dst", "device_dst"])
def test_foreign_corpus_in_one_call(eng, foreign, device):
    rc, text, dst_off, status = raw_inflate(eng, [m for _, m, _ in foreign], device)
    assert rc == 0, eng._err()
    assert (status == 0).all(), [foreign[k][0] for k in np.nonzero(status)[0]]
    check_valid(text, dst_off, status, [d for _, _, d in foreign])


@pytest.mark.parametrize("device", [False, True], ids=["host_dst", "device_dst"])
def test_foreign_corpus_one_member_per_call(eng, foreign, device):
    for name, m, d in foreign:
        rc, text, dst_off, status = raw_inflate(eng, [m], device)
        assert rc == 0 and status.tolist() == [0], (name, status, eng._err())
        check_valid(text, dst_off, status, [d])


@pytest.mark.parametrize("device", [False, True], ids=["host_dst", "device_dst"])
def test_foreign_damaged_members_between_valid_ones(eng, foreign, device, tmp_path):
    """bc.foreign_damaged() interleaved with valid foreign members: every status is the CPU core's (which test_bgzf_cpu.py holds
    to zlib, category included), the neighbours' bytes and the guards are intact, the engine goes on serving lrt()."""
    import basevar_amd as bv
    from basevar_amd.synth import make_slab
    damaged = bc.foreign_damaged()
    p, rows = bc.core_verdicts(bc.build_core_check(tmp_path), [m for _, m in damaged], tmp_path)
    assert p.returncode == 0 and len(rows) == len(damaged), p.stderr[-2000:]
    good = [(m, d) for _, m, d in foreign if len(d) > 0]
    members, expect, datas = [], [], []
    for k, ((name, m), r) in enumerate(zip(damaged, rows)):
        assert r[0] == bc.FOREIGN_DAMAGED_EXPECT[name], (name, r)
        g = good[(7 * k) % len(good)]
        members += [g[0], m]
        expect += [0, r[0]]
        datas += [g[1], None]
    members.append(good[0][0]); expect.append(0); datas.append(good[0][1])
    slab = make_slab(48, 20000, seed=5, coverage=0.08, n_groups=2)
    fresh = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(20000), device=0)
    try:
        exp = fresh.lrt(slab)
    finally:
        fresh.close()
    rc, text, dst_off, status = raw_inflate(eng, members, device)
    assert rc == 0, eng._err()
    wrong = [(k, damaged[k // 2][0] if k % 2 else "valid", int(status[k]), e) for k, e in enumerate(expect) if status[k] != e]
    assert not wrong, wrong[:20]
    assert len(set(status.tolist())) == 5
    for k, d in enumerate(datas):
        lo, hi = int(dst_off[k]), int(dst_off[k + 1])
        if d is not None:
            assert text[GUARD + lo:GUARD + hi].tobytes() == d, k
        elif status[k] == 0:
            assert text[GUARD + lo:GUARD + hi].tobytes() == zlib.decompress(bc.payload_of(members[k]), -15), k
    assert (text[:GUARD] == 0xA5).all() and (text[GUARD + int(dst_off[-1]):] == 0xA5).all()
    got = eng.lrt(slab)
    assert got.sites.tobytes() == exp.sites.tobytes() and got.groups.tobytes() == exp.groups.tobytes()
    assert got.n_variant == exp.n_variant and exp.n_variant > 0


def test_every_destination_alignment_and_text_size(eng, foreign):
    """The write-out splits a member's text into head bytes, 16-byte lines and tail bytes by where it lands.  Members ordered so
    that every pair (destination address mod 16, text size) occurs for the sizes 0 .. 33, 47, 48, 49 and 65 536: the pairs are
    computed from the tensor's address, GUARD and the dst_off the call returned, and the set is complete before a byte is read."""
    import torch
    by_size = {len(d): (m, d) for n, m, d in foreign if n.startswith("size/")}
    sizes = list(range(34)) + [47, 48, 49, 65536]
    dst = torch.full((2 * GUARD + 16 * sum(s + 16 for s in sizes),), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    base = (dst.data_ptr() + GUARD) % 16
    members, datas, at = [], [], 0
    for s in sizes:
        for a in range(16):
            fill = (a - base - at) % 16  # a member of that many bytes moves the next one to alignment a
            for size in ([fill] if fill else []) + [s]:
                members.append(by_size[size][0]); datas.append(by_size[size][1])
                at += size
    rc, text, dst_off, status = raw_inflate(eng, members, True, dst=dst)
    assert rc == 0, eng._err()
    pairs = {((dst.data_ptr() + GUARD + int(dst_off[k])) % 16, int(dst_off[k + 1] - dst_off[k])) for k in range(len(members))}
    assert pairs >= {(a, s) for a in range(16) for s in sizes}
    check_valid(text, dst_off, status, datas)


@pytest.mark.parametrize("device", [False, True], ids=["host_dst", "device_dst"])
def test_foreign_corpus_across_staging_slots(eng, foreign, device, monkeypatch):
    """a chunk of 70 000 compressed bytes: the foreign corpus, eight times over, crosses both staging slots many times, and the
    payloads start at every offset mod 4 inside their chunk (the packing rule of bv_inflate.hip: a chunk takes members while
    their bytes fit it and their text fits four times that)"""
    chunk = 70000
    monkeypatch.setenv("BASEVAR_AMD_TEXT_CHUNK_BYTES", str(chunk))
    members = [m for _, m, _ in foreign] * 8
    datas = [d for _, _, d in foreign] * 8
    starts, n_chunks, used_in, used_out = set(), 1, 0, 0
    for m, d in zip(members, datas):
        if used_in and (used_in + len(m) > chunk or used_out + len(d) > 4 * chunk):
            n_chunks, used_in, used_out = n_chunks + 1, 0, 0
        starts.add((used_in + 12 + int.from_bytes(m[10:12], "little")) % 4)
        used_in, used_out = used_in + len(m), used_out + len(d)
    assert starts == {0, 1, 2, 3} and n_chunks > 20
    rc, text, dst_off, status = raw_inflate(eng, members, device)
    assert rc == 0, eng._err()
    check_valid(text, dst_off, status, datas)
