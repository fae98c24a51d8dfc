"""GPU tests of bv_engine_pileup / _fetch / _rows (include/basevar_amd_pileup.h): the planes, depths and tokens the device piles up
are, byte for byte, those of the stand-alone harness tests/cpp/pileup_core_check.cpp -- host/pileup.hpp's, which the harness has
held to basevar_amd/csrc/bv_pileup_core.h on the way -- at the sample counts, window sizes and read lengths at which the kernels
of basevar_amd/csrc/bv_pileup.hip can go wrong; nothing outside the fetched buffers is touched; the gathered rows give
bv_engine_submit's records of the host-built slab."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_py  # noqa: E402
import pileup_ref as pr  # noqa: E402

SENTINEL = 0xA5
N_MAX = 300


@pytest.fixture(scope="module")
def harness():
    return pr.build()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return pr.Corpus(tmp_path_factory.mktemp("pileup_corpus"), N_MAX)


@pytest.fixture(scope="module")
def dumps(harness, corpus, tmp_path_factory):
    """the harness's result for (n samples, window), computed once and left unchanged"""
    d, cache = tmp_path_factory.mktemp("pileup_dumps"), {}

    def get(n, name):
        if (n, name) not in cache:
            cache[(n, name)] = pr.run_bam(harness, d / ("%d_%s.bin" % (n, name)), corpus, n, pr.WINDOWS[name])[0]
        return cache[(n, name)]
    return get


def engine(corpus=None, max_sites=1024, n=N_MAX):
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=max_sites, min_af_value=bv.min_af(max(n, 1)), device=0, max_samples=max(n, 1))
    if corpus is not None:
        e.pileup_set_reference(corpus.fa)
    return e


def pile(eng, d, window, pitch=None, device=False, n=None):
    import torch
    rec = torch.from_numpy(d.records).cuda() if device else d.records
    if device:
        torch.cuda.synchronize()
    return eng.pileup(rec, d.run_off, d.run_sample, n or d.n_samples, d.tid, pr.REGION, window, pr.MAPQ_THD, pitch=pitch)


def check(got, d, n_cov):
    """the fetched pileup against the harness's, byte for byte; cells at or beyond n_samples are uncovered"""
    n = d.n_samples
    assert n_cov == d.n_covered
    for f in ("cell", "qual", "mapq", "rank"):
        assert got[f].shape[0] == d.rows and got[f].shape[1] % 16 == 0
        assert got[f][:, :n].tobytes() == getattr(d, f)[:, :n].tobytes(), f
    assert (got["cell"][:, n:] == 8).all() and not got["qual"][:, n:].any() and not got["mapq"][:, n:].any() and not got["rank"][:, n:].any()
    assert got["depth"].tobytes() == d.depth.tobytes()
    assert got["tokens"].tobytes() == d.tokens.tobytes() and got["text"].tobytes() == d.text.tobytes()


def pile_and_check(eng, d, window, **kw):
    n_cov = pile(eng, d, window, **kw)
    check(eng.pileup_fetch(), d, n_cov)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, N_MAX])
def test_planes_depths_tokens_are_the_harnesss(corpus, dumps, n):
    """1,000 rows at every sample count; pitch n rounded to 16 and a wider one, host and device records"""
    d = dumps(n, "w1000")
    assert d.n_tokens > 0 and d.n_covered > 500
    eng = engine(corpus)
    check_rows = lambda **kw: pile_and_check(eng, d, pr.WINDOWS["w1000"], **kw)
    check_rows()
    assert eng.pileup_fetch()["cell"].shape[1] == (n + 15) // 16 * 16
    check_rows(pitch=(n + 15) // 16 * 16 + 48, device=True)
    check_rows(device=True)
    eng.close()


@pytest.mark.parametrize("name", ["w1", "w2", "w64", "w65", "edge", "next"])
def test_small_windows_and_the_steps_edge(corpus, dumps, name):
    d = dumps(65, name)
    eng = engine(corpus)
    pile_and_check(eng, d, pr.WINDOWS[name], device=(name in ("w2", "edge")))
    eng.close()


def test_a_small_window_behind_a_large_one_has_no_stale_cells(corpus, dumps):
    eng = engine(corpus)
    for name, n in (("w1000", 65), ("w1", 65), ("w1000", 2), ("w2", 65)):
        d = dumps(n, name)
        pile_and_check(eng, d, pr.WINDOWS[name])
    eng.close()


def test_records_cross_the_link_in_chunks(corpus, dumps, monkeypatch):
    """host records larger than the staging chunk: every chunk boundary inside a record"""
    monkeypatch.setenv("BASEVAR_AMD_PILEUP_CHUNK", "1000")
    d = dumps(65, "w1000")
    assert d.records.size > 20 * 1000
    eng = engine(corpus)
    pile_and_check(eng, d, pr.WINDOWS["w1000"])
    eng.close()


def test_the_largest_window(corpus, dumps):
    """bv_pileup_max_rows() rows, the whole first step and the `seen` bits at their largest: a cell does not depend on the window
    it is piled up in, so the rows of the smaller windows are the harness's"""
    from basevar_amd import _capi
    w = (1, _capi.load().bv_pileup_max_rows())
    assert w[1] == pr.STEP
    eng = engine(corpus)
    d0 = dumps(2, "w1000")
    n_cov = pile(eng, d0, w, pitch=16)  # (the runs of the small window: the reads that reach it; the edge's are piled up below)
    got = eng.pileup_fetch()
    assert got["cell"].shape == (pr.STEP, 16) and n_cov == int((got["depth"] > 0).sum()) >= d0.n_covered
    for name in ("w1000", "w64", "w1"):
        d = dumps(2, name)
        lo, hi = pr.WINDOWS[name][0] - 1, pr.WINDOWS[name][1]
        for f in ("cell", "qual", "mapq", "rank"):
            assert got[f][lo:hi, :2].tobytes() == getattr(d, f)[:, :2].tobytes(), (name, f)
        assert got["depth"][lo:hi].tobytes() == d.depth.tobytes()
    d = dumps(2, "edge")
    pile(eng, d, w, pitch=16)
    got = eng.pileup_fetch()
    lo, hi = pr.WINDOWS["edge"][0] - 1, pr.WINDOWS["edge"][1]
    for f in ("cell", "qual", "mapq", "rank"):
        assert got[f][lo:hi, :2].tobytes() == getattr(d, f)[:, :2].tobytes(), f
    assert int(got["depth"][-1]) > 0
    eng.close()


def test_no_runs_is_an_empty_pileup(corpus):
    eng = engine(corpus)
    n_cov = eng.pileup(b"", [], [], 5, pr.TID, pr.REGION, (1000, 1063), pr.MAPQ_THD)
    got = eng.pileup_fetch()
    assert n_cov == 0 and got["cell"].shape == (64, 16) and (got["cell"] == 8).all() and not got["rank"].any() and not got["depth"].any()
    assert got["tokens"].size == 0 and got["text"].size == 0
    slab, pos, depth = eng.pileup_rows()
    assert slab.n_sites == 0 and slab.n_samples == 5 and pos.size == 0
    eng.close()


def test_fetch_writes_its_buffers_and_nothing_else(corpus, dumps):
    """sentinels around every fetched buffer, host and device; a capacity that is too small: the sizes, and nothing written"""
    import torch
    from basevar_amd import _capi
    lib = _capi.load()
    d = dumps(65, "w1000")
    eng = engine(corpus)
    pile(eng, d, pr.WINDOWS["w1000"])
    cells, pad = d.rows * 80, 64
    sizes = dict(cell=cells, qual=cells, mapq=cells, rank=2 * cells, depth=4 * d.rows, tokens=24 * d.n_tokens, text=int(d.text_bytes))
    for dev in (False, True):
        bufs = {k: np.full(v + 2 * pad, SENTINEL, np.uint8) for k, v in sizes.items()}
        if dev:
            bufs = {k: torch.from_numpy(v).cuda() for k, v in bufs.items()}
        res = _capi.PileupResult()
        res.mem_kind = _capi.BV_MEM_DEVICE if dev else _capi.BV_MEM_HOST
        for k, v in bufs.items():
            setattr(res, k, (int(v.data_ptr()) if dev else v.ctypes.data) + pad)
        # one token too few: refused, nothing written, the sizes reported
        res.cells_capacity, res.rows_capacity, res.tokens_capacity, res.text_capacity = cells, d.rows, d.n_tokens - 1, int(d.text_bytes)
        assert lib.bv_engine_pileup_fetch(eng._h, C.byref(res), None) == _capi.BV_ERR_INVALID_ARG and b"capacity" in lib.bv_last_error(eng._h)
        assert (res.cells, res.rows, res.n_tokens, res.text_bytes) == (cells, d.rows, d.n_tokens, d.text_bytes)
        host = {k: (v.cpu().numpy() if dev else v) for k, v in bufs.items()}
        assert all((v == SENTINEL).all() for v in host.values())
        res.tokens_capacity = d.n_tokens
        assert lib.bv_engine_pileup_fetch(eng._h, C.byref(res), None) == 0
        host = {k: (v.cpu().numpy() if dev else v) for k, v in bufs.items()}
        for k, v in host.items():
            assert (v[:pad] == SENTINEL).all() and (v[pad + sizes[k]:] == SENTINEL).all(), k
        body = lambda k: host[k][pad:pad + sizes[k]]
        got = dict(cell=body("cell").reshape(d.rows, 80), qual=body("qual").reshape(d.rows, 80), mapq=body("mapq").reshape(d.rows, 80),
                   rank=body("rank").view("<u2").reshape(d.rows, 80), depth=body("depth").view("<u4"), tokens=body("tokens").view(pr.TOKEN_DTYPE), text=body("text"))
        check(got, d, d.n_covered)
    eng.close()


def test_records_inflated_on_the_device_are_piled_up_where_they_lie(corpus, dumps):
    """the BAM files' BGZF members inflated by bgzf_inflate to a device buffer; each file's records (behind its header) are a run"""
    import torch
    n = 5
    d = dumps(n, "w1000")
    eng = engine(corpus)
    members, member_off, run_at = [], [0], []
    for path in corpus.bams[:n]:
        blocks = bam_py.bgzf_blocks(path)
        raw = b"".join(p for _, _, p in blocks)
        l_text, = struct.unpack_from("<i", raw, 4)
        o = 8 + l_text
        n_ref, = struct.unpack_from("<i", raw, o)
        o += 4
        for _ in range(n_ref):
            l_name, = struct.unpack_from("<i", raw, o)
            o += 8 + l_name
        run_at.append((o, len(raw)))
        data = open(path, "rb").read()
        for off, total, _ in blocks[:-1]:  # (without the end-of-file marker, which holds nothing)
            members.append(data[off:off + total])
            member_off.append(member_off[-1] + total)
    total = sum(e for _, e in run_at)
    dst = torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    _, dst_off, status = eng.bgzf_inflate(b"".join(members), member_off, dst_ptr=int(dst.data_ptr()), dst_capacity=total)
    assert not status.any() and int(dst_off[-1]) == total
    run_off, run_sample, base = [], [], 0
    for s, (hdr, size) in enumerate(run_at):
        if size > hdr:
            run_off.append(base + hdr)
            run_sample.append(s)
        base += size
    # a file's header lies between two files' records and a run ends where the next begins: the records are put back to back by a
    # copy on the device; nothing comes back to the host
    parts = [dst[o:o + (run_at[s][1] - run_at[s][0])] for o, s in zip(run_off, run_sample)]
    packed = torch.cat(parts)
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([int(p.numel()) for p in parts])
    torch.cuda.synchronize()
    n_cov = eng.pileup(packed, off, run_sample, n, pr.TID, pr.REGION, pr.WINDOWS["w1000"], pr.MAPQ_THD)
    check(eng.pileup_fetch(), d, n_cov)
    assert (dst[total:].cpu().numpy() == SENTINEL).all()
    eng.close()


def host_slab(d, fa, window, tagged):
    """the covered rows of the harness's planes as bv_call builds its slab from a PileupTile"""
    from basevar_amd.synth import tag_ranks
    rows = np.flatnonzero(d.depth)
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    slab = dict(base_strand=d.cell[rows], qual=d.qual[rows], mapq=d.mapq[rows], rpr=d.rank[rows], n_samples=d.n_samples,
                ref_base=np.array([code.get(fa[window[0] + int(r) - 1].upper(), 4) for r in rows], np.uint8))
    return (tag_ranks(slab) if tagged else slab), rows


@pytest.mark.parametrize("tagged", [False, True])
def test_gathered_rows_give_the_records_of_the_host_built_slab(corpus, dumps, tagged):
    d = dumps(65, "w1000")
    w = pr.WINDOWS["w1000"]
    eng = engine(corpus)
    slab, rows = host_slab(d, corpus.fa, w, tagged)
    want = eng.lrt(slab)
    got = eng.lrt_pileup(d.records, d.run_off, d.run_sample, d.n_samples, d.tid, pr.REGION, w, pr.MAPQ_THD, tagged=tagged)
    assert got.sites.tobytes() == want.sites.tobytes() and got.n_variant == want.n_variant and len(got.sites) == d.n_covered
    assert (got.positions == w[0] + rows).all() and (got.depth == d.depth[rows]).all()
    assert got.tokens == {(int(t["pos"]), int(t["sample"])): d.text[int(t["text_off"]):int(t["text_off"]) + int(t["text_len"])].tobytes() for t in d.tokens}
    s, pos, depth = eng.pileup_rows(tagged=tagged)
    assert (s.n_sites, s.n_samples, s.pitch, s.mem_kind, s.layout, s.n_groups) == (len(rows), 65, 80, 0, 1 if tagged else 0, 0) and not s.group_id
    assert (pos == got.positions).all() and (depth == got.depth).all()
    eng.close()


def test_tagging_is_refused_for_a_rank_beyond_8191(corpus):
    from basevar_amd import _capi
    rng = np.random.default_rng(3)
    long_read = pr.record_bytes(pr.read(rng, 999, [(pr.M, 8200)]))
    eng = engine(corpus, max_sites=9000, n=1)
    w = (1000, 9999)
    assert eng.pileup(long_read, [0, len(long_read)], [0], 1, pr.TID, pr.REGION, w, pr.MAPQ_THD) == 8200
    with pytest.raises(RuntimeError, match="tagged layout") as ei:
        eng.pileup_rows(tagged=True)
    assert ei.value.args[1] == _capi.BV_ERR_INVALID_ARG
    slab, pos, depth = eng.pileup_rows(tagged=False)
    assert slab.n_sites == 8200 and int(pos[-1]) == 9199 and int(eng.pileup_fetch()["rank"][8199, 0]) == 8200
    eng.close()


def test_refusals(corpus, dumps, harness, tmp_path):
    """each returns its status and message; the engine then holds no pileup"""
    from basevar_amd import _capi
    d = dumps(2, "w64")
    w = pr.WINDOWS["w64"]
    eng = engine(None)

    def refused(status, text, **kw):
        a = dict(records=d.records, run_off=d.run_off, run_sample=d.run_sample, n_samples=2, tid=d.tid, region=pr.REGION, window=w, mapq_thd=pr.MAPQ_THD)
        a.update(kw)
        with pytest.raises(RuntimeError, match=text) as ei:
            eng.pileup(**a)
        assert ei.value.args[1] == status
        with pytest.raises(RuntimeError, match="no completed bv_engine_pileup"):
            eng.pileup_fetch()
        with pytest.raises(RuntimeError, match="no completed bv_engine_pileup"):
            eng.pileup_rows()

    refused(_capi.BV_ERR_INVALID_ARG, "no reference set")
    eng.pileup_set_reference(corpus.fa)
    pile(eng, d, w)
    refused(_capi.BV_ERR_INVALID_ARG, "step grid", window=(499990, 500010))
    refused(_capi.BV_ERR_INVALID_ARG, "step grid", window=(1363, 1300))
    refused(_capi.BV_ERR_INVALID_ARG, "step grid", region=(1200, 1350))
    off = d.run_off.copy()
    off[1] = off[2] + 1
    refused(_capi.BV_ERR_INVALID_ARG, "run_off out of order", run_off=off)
    refused(_capi.BV_ERR_INVALID_ARG, "run_sample descends", run_sample=d.run_sample[::-1].copy())
    refused(_capi.BV_ERR_INVALID_ARG, "beyond n_samples", n_samples=1)
    refused(_capi.BV_ERR_TOO_LARGE, "bv_pileup_max_rows", window=(1, 500001))
    refused(_capi.BV_ERR_INVALID_ARG, "reserved_", reserved=1)
    refused(_capi.BV_ERR_INVALID_ARG, "pitch", pitch=24)
    refused(_capi.BV_ERR_INVALID_ARG, "beyond the reference", region=(1, 700000), window=(599990, 600001))
    # five damaged runs that the CPU build is held to (tests/test_pileup_core_cpu.py): the same status, sample, run and offset
    rng = np.random.default_rng(9)
    good = [pr.record_bytes(pr.read(rng, 1300 + 3 * k, [(pr.S, 1), (pr.I, 1), (pr.M, 3)])) for k in range(3)]
    patched = lambda b, at, fmt, v: b[:at] + np.array([v], fmt).tobytes() + b[at + np.dtype(fmt).itemsize:]
    damaged = [good[0] + patched(good[1], 0, "<u4", 31), good[0] + good[1][:-1], good[0] + patched(good[1], 4 + 16, "<i4", 1 << 20),
               good[0] + pr.record_bytes(pr.read(rng, 1310, [(pr.M, 50)], seq="ACGTACGTAC", qual=[30] * 10)),
               good[0] + patched(good[1], 4 + 12, "<u2", 60000)]
    for k, run in enumerate(damaged):
        want, _ = pr.run_raw(harness, tmp_path / "raw.bin", tmp_path, corpus.fa, [good[2], run], [0, 1], 2, w)
        assert want.status != 0 and (want.fail_sample, want.fail_run, want.fail_at) == (1, 1, len(good[0]))
        both = np.frombuffer(good[2] + run, np.uint8)
        refused(_capi.BV_ERR_DATA, "sample 1, run 1, the record at byte %d of the run: " % len(good[0]), records=both,
                run_off=[0, len(good[2]), both.size], run_sample=[0, 1])
        assert pr.BAD_BLOCK <= want.status <= pr.BAD_QUERY
    # the unknown base letter: BV_ERR_SITE with the host's text
    bad = pr.record_bytes(pr.read(rng, 1350, [(pr.M, 40)], seq="ACGT" * 7 + "ACM" + "ACGTACGTA"))
    with pytest.raises(RuntimeError) as ei:
        eng.pileup(bad, [0, len(bad)], [0], 1, pr.TID, pr.REGION, w, pr.MAPQ_THD)
    assert ei.value.args[1] == _capi.BV_ERR_SITE and pr.BAD_BASE_TEXT in str(ei.value.args[0])
    # ... and the engine is as good as before
    pile_and_check(eng, d, w)
    eng.close()
