"""GPU tests of the device pileup on raw runs (pileup_raw_cases.py): wave_walk of basevar_amd/csrc/bv_pileup.hip is a second
statement of bv_pileup_walk, and here it is held to the first -- the stand-alone harness tests/cpp/pileup_core_check.cpp in its
`raw` mode -- byte for byte, on a seeded campaign of runs (several runs a sample, empty runs, leading samples without runs, records
at an offset inside a larger buffer, every operation code, quals 0 and 255, token texts longer than a wave) and on hand-built
cases; at the sample counts where the depth and gather kernels' row loops take further steps; through bv_engine_pileup_submit
called directly; at the tagging boundary; and on a read of 66,000 bases.  Every input sent here has first gone through the core
under ASan + UBSan in tests/test_pileup_core_cpu.py, on the same bytes."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_py  # noqa: E402
import pileup_ref as pr  # noqa: E402
import pileup_raw_cases as rc  # noqa: E402
from test_gpu_pileup import check, engine, host_slab  # noqa: E402

SENTINEL = 0xA5
NO_PILEUP = "no completed bv_engine_pileup"


@pytest.fixture(scope="module")
def harness():
    return pr.build()


@pytest.fixture(scope="module")
def dumps(harness, tmp_path_factory):
    """the harness's result for a case, computed once per key and left unchanged"""
    tmp, cache = tmp_path_factory.mktemp("pileup_raw_dumps"), {}

    def get(key, case):
        if key not in cache:
            runs, run_sample, n, window, ref = case
            cache[key] = pr.run_raw(harness, tmp / "d.bin", tmp, ref, runs, run_sample, n, window)[0]
        return cache[key]
    return get


@pytest.fixture(scope="module")
def eng():
    """one engine for the whole campaign: a small pileup follows a large one, one with tokens follows one without"""
    e = engine(None, n=130)
    yield e
    e.close()


def pile(eng, case, where="host", offset=0, pitch=None):
    """the case's runs piled up: records on the host or the device, `offset` bytes into a larger buffer with sentinels around"""
    import torch
    runs, run_sample, n, window, ref = case
    body = np.frombuffer(b"".join(runs), np.uint8)
    tail = 64 if offset else 0
    buf = np.full(offset + body.size + tail, SENTINEL, np.uint8)
    buf[offset:offset + body.size] = body
    off = np.zeros(len(runs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in runs])
    off += np.uint64(offset)
    rec = buf
    if where == "device":
        rec = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
    n_cov = eng.pileup(rec, off, run_sample, n, pr.TID, pr.REGION, window, pr.MAPQ_THD, pitch=pitch)
    back = rec.cpu().numpy() if where == "device" else rec
    assert (back[:offset] == SENTINEL).all() and (back[offset + body.size:] == SENTINEL).all() and back[offset:offset + body.size].tobytes() == body.tobytes()
    return n_cov


def pile_and_check(eng, case, d, **kw):
    n_cov = pile(eng, case, **kw)
    got = eng.pileup_fetch()
    check(got, d, n_cov)
    return got


# ----------------------------------------------------------------------------------------------------------------- 1. the campaign
@pytest.mark.parametrize("block", range(len(rc.SEED_BLOCKS)))
def test_campaign(eng, dumps, block):
    """every round from host records; every third also from a device tensor; every third at an odd offset inside a larger buffer,
    host and device: run_off[0] != 0"""
    for seed in rc.SEED_BLOCKS[block]:
        case = rc.campaign_round(seed)
        d = dumps(("campaign", seed), case)
        assert d.status == 0
        eng.pileup_set_reference(case[4])
        pile_and_check(eng, case, d)
        if seed % 3 == 0:
            pile_and_check(eng, case, d, where="device")
        if seed % 3 == 1:
            pile_and_check(eng, case, d, offset=37)
            pile_and_check(eng, case, d, where="device", offset=4099, pitch=(case[2] + 15) // 16 * 16 + 48)


# -------------------------------------------------------------------------------------------------------------- 2. directed cases
def as_dump(got):
    return types.SimpleNamespace(**got)


VALID = sorted(k for k, c in rc.directed().items() if not c.status)
DAMAGED = sorted(k for k, c in rc.directed().items() if c.status)


@pytest.mark.parametrize("name", VALID)
def test_directed_case(eng, dumps, name):
    """the harness's result, and what the case itself states of its answer"""
    c = rc.directed()[name]
    d = dumps(("directed", name), c.tuple())
    assert d.status == 0
    eng.pileup_set_reference(c.ref)
    got = pile_and_check(eng, c.tuple(), d)
    rc.check_expectation(c, as_dump(got))
    pile_and_check(eng, c.tuple(), d, where="device", offset=1)


def refused(eng, case, status, text):
    with pytest.raises(RuntimeError, match=text) as ei:
        pile(eng, case)
    assert ei.value.args[1] == status
    with pytest.raises(RuntimeError, match=NO_PILEUP):
        eng.pileup_fetch()
    with pytest.raises(RuntimeError, match=NO_PILEUP):
        eng.pileup_rows()


def refusal_of(d):
    from basevar_amd import _capi
    where = "sample %d, run %d, the record at byte %d of the run" % (d.fail_sample, d.fail_run, d.fail_at)
    if d.status == pr.BAD_BASE:
        return _capi.BV_ERR_SITE, "Why dose the size of aligned base is not 1.*" + where
    return _capi.BV_ERR_DATA, where + ": "


def test_damaged_cases_are_refused_with_the_harnesss_place(eng, dumps):
    """BV_ERR_DATA with the harness's sample, run and offset (of two failing samples the lower one's), BV_ERR_SITE with the host's
    text; then no pileup is held; after all of them a good pileup is the harness's"""
    from basevar_amd import _capi
    assert {rc.directed()[k].status for k in DAMAGED} == {1, 2, 3, 4, 5, 6}
    for name in DAMAGED:
        c = rc.directed()[name]
        d = dumps(("directed", name), c.tuple())
        assert d.status == c.status and (d.fail_sample, d.fail_run, d.fail_at) == c.expect["fail"]
        eng.pileup_set_reference(c.ref)
        if d.status == pr.BAD_REF:
            # an anchor outside the reference needs a window that ends beyond it: refused on the host, before any launch
            refused(eng, c.tuple(), _capi.BV_ERR_INVALID_ARG, "beyond the reference")
        else:
            refused(eng, c.tuple(), *refusal_of(d))
    good = rc.directed()["long_insertions"]
    eng.pileup_set_reference(good.ref)
    pile_and_check(eng, good.tuple(), dumps(("directed", "long_insertions"), good.tuple()))


def test_truncation_at_every_byte(eng, dumps):
    """a three-record run cut at every byte: the records before the cut are piled up, or BV_ERR_DATA at the record that is cut"""
    fa = rc.FA[:4000].encode()
    eng.pileup_set_reference(fa)
    for cut, run, status, start in rc.truncations():
        case = ([run], [0], 1, (1000, 1063), fa)
        d = dumps(("cut", cut), case)
        assert d.status == status
        if status:
            assert (d.fail_sample, d.fail_run, d.fail_at) == (0, 0, start)
            refused(eng, case, *refusal_of(d))
        else:
            pile_and_check(eng, case, d)


# ----------------------------------------------------------------------------- 3. sample counts at which the row loops step again
@pytest.mark.parametrize("n", [512, 513, 1040, 4096, 4097, 4113, 20000])
def test_sample_counts_at_which_the_row_loops_take_further_steps(dumps, n):
    """bv_pileup_depth_kernel takes a second step from 513 samples on, bv_pileup_gather_kernel from 4,097: planes, depths and
    tokens at the default pitch and a wider one; the largest rank, which lies in the row's last cell, through the tagging boundary"""
    case = rc.wide_round(n)
    d = dumps(("wide", n), case)
    assert d.status == 0 and d.n_tokens > 3 and d.n_covered == d.rows and int(d.rank[-1, n - 1]) == 8191 == int(d.rank.max())
    e = engine(None, n=n)
    e.pileup_set_reference(case[4])
    pile_and_check(e, case, d, pitch=(n + 15) // 16 * 16 + 48, where="device")
    got = pile_and_check(e, case, d)
    assert got["cell"].shape[1] == (n + 15) // 16 * 16
    slab, pos, depth = e.pileup_rows(tagged=True)  # 8,191 fits
    assert (slab.n_sites, slab.layout) == (d.rows, 1) and (depth == d.depth).all() and (pos == case[3][0] + np.arange(d.rows)).all()
    pile(e, rc.wide_round(n, long_rank=8192))
    with pytest.raises(RuntimeError, match="rank of 8192 does not fit the tagged layout"):
        e.pileup_rows(tagged=True)
    e.close()


# ------------------------------------------------------------------------ 4. the gathered slab and bv_engine_pileup_submit, directly
def submit(e, first, n, n_samples, group_id=None, n_groups=0, with_gout=True):
    from basevar_amd import _capi
    out = np.zeros(n, _capi.SITE_DTYPE)
    gout = np.zeros((n, n_groups), _capi.GROUP_DTYPE) if n_groups and with_gout else None
    cell, phred = np.full((n, n_samples), SENTINEL, np.uint8), np.full((n, n_samples), SENTINEL, np.uint8)
    rc_ = e._lib.bv_engine_pileup_submit(e._h, first, n, group_id.ctypes.data if group_id is not None else None, n_groups, out.ctypes.data if n else None,
                                         gout.ctypes.data if gout is not None else None, cell.ctypes.data if n else None, phred.ctypes.data if n else None, None)
    return rc_, out, gout, cell, phred


@pytest.mark.parametrize("tagged", [False, True])
@pytest.mark.parametrize("n", [65, 4113])
def test_submit_of_the_gathered_slab(dumps, n, tagged):
    """65 samples: the wave-per-row kernels; 4,113: the fused short-row kernel and the gather's second step.  Most rows are variant
    sites, so the rank-sum fields read the slab's mapq and rpr planes.  Records and group records of any sub-range are those of the
    host-built slab's rows (a record does not depend on the rest of its launch); cell / phred are the harness's rows"""
    from basevar_amd import _capi
    case = rc.variant_round(n)
    runs, run_sample, _, window, ref = case
    d = dumps(("variant", n), case)
    slab, rows = host_slab(d, ref.decode(), window, tagged)
    n_cov = len(rows)
    assert d.status == 0 and 250 <= n_cov <= 300
    gid = np.random.default_rng(n).integers(0, 3, n).astype(np.uint8)
    e = engine(None, n=n)
    e.pileup_set_reference(ref)
    want = {0: e.lrt(slab), 3: e.lrt(dict(slab, group_id=gid, n_groups=3))}
    assert want[0].n_variant > n_cov // 2
    assert pile(e, case) == n_cov
    # a submit before pileup_rows
    rc_, *_ = submit(e, 0, 1, n)
    assert rc_ == _capi.BV_ERR_INVALID_ARG and b"no bv_engine_pileup_rows since the last pileup" in e._lib.bv_last_error(e._h)
    s, pos, depth = e.pileup_rows(tagged=tagged)
    assert (s.n_sites, s.n_samples, s.layout) == (n_cov, n, 1 if tagged else 0) and (pos == window[0] + rows).all() and (depth == d.depth[rows]).all()
    for n_groups in (0, 3):
        for first, cnt in ((0, n_cov), (1, 1), (n_cov - 1, 1), (3, 37)):
            rc_, out, gout, cell, phred = submit(e, first, cnt, n, gid if n_groups else None, n_groups)
            assert rc_ == 0, e._lib.bv_last_error(e._h)
            assert out.tobytes() == want[n_groups].sites[first:first + cnt].tobytes(), (n_groups, first, cnt)
            if n_groups:
                assert gout.tobytes() == want[3].groups[first:first + cnt].tobytes(), (first, cnt)
            assert cell.tobytes() == d.cell[rows[first:first + cnt], :n].tobytes() and phred.tobytes() == d.qual[rows[first:first + cnt], :n].tobytes()
    for args, text in (((n_cov - 1, 2), b"beyond the slab"), ((n_cov, 1), b"beyond the slab"), ((0, 0), b"n == 0")):
        rc_, *_ = submit(e, args[0], args[1], n)
        assert rc_ == _capi.BV_ERR_INVALID_ARG and text in e._lib.bv_last_error(e._h), args
    rc_, *_ = submit(e, 0, 2, n, gid, 3, with_gout=False)
    assert rc_ == _capi.BV_ERR_INVALID_ARG and b"null out/gout/group_id" in e._lib.bv_last_error(e._h)
    # ... and the slab is as good as before
    rc_, out, *_ = submit(e, 3, 37, n)
    assert rc_ == 0 and out.tobytes() == want[0].sites[3:40].tobytes()
    e.close()


# ----------------------------------------------------------------------------------------------------------- 5. the tagging boundary
def test_tagging_boundary_at_8191(dumps):
    rng = np.random.default_rng(3)
    fa = rc.FA[:12000].encode()
    w = (1000, 9999)
    e = engine(None, max_sites=9000, n=1)
    e.pileup_set_reference(fa)
    rec = pr.record_bytes(pr.read(rng, 999, [(pr.M, 8191)]))
    args = (rec, [0, len(rec)], [0], 1, pr.TID, pr.REGION, w, pr.MAPQ_THD)
    plain = e.lrt_pileup(*args, tagged=False)
    tagged = e.lrt_pileup(*args, tagged=True)
    assert len(plain.sites) == 8191 and tagged.sites.tobytes() == plain.sites.tobytes() and int(e.pileup_fetch()["rank"][8190, 0]) == 8191
    rec = pr.record_bytes(pr.read(rng, 999, [(pr.M, 8192)]))
    assert e.pileup(rec, [0, len(rec)], [0], 1, pr.TID, pr.REGION, w, pr.MAPQ_THD) == 8192
    with pytest.raises(RuntimeError, match="rank of 8192 does not fit the tagged layout"):
        e.pileup_rows(tagged=True)
    slab, pos, depth = e.pileup_rows(tagged=False)
    assert slab.n_sites == 8192 and slab.layout == 0 and int(pos[-1]) == 9191
    e.close()


# -------------------------------------------------------------------------------------------------------------------- 6. the long read
def test_a_read_of_66000_bases(harness, tmp_path):
    """the cell of query index 65,535 (position 66,536) stays claimed: rank 65,535, saturated, and depth counts it"""
    read = rc.long_read()
    w = (66500, 66600)
    path, fasta = str(tmp_path / "long.bam"), str(tmp_path / "ref.fa")
    bam_py.write_bam(path, pr.REFS, [read])
    pr.write_fasta(fasta, rc.FA)
    d, _ = pr.run_bam(harness, tmp_path / "l.bin", None, 1, w, bams=[path], fasta=fasta)  # (host against core on the way)
    assert d.status == 0 and d.n_covered == d.rows == 101 and int(d.rank[36, 0]) == 65535 == int(d.rank[35, 0]) and int(d.rank[34, 0]) == 65534
    e = engine(None, n=1)
    e.pileup_set_reference(rc.FA)
    n_cov = e.pileup(d.records, d.run_off, d.run_sample, 1, d.tid, pr.REGION, w, pr.MAPQ_THD)
    check(e.pileup_fetch(), d, n_cov)
    assert n_cov == 101
    e.close()


def test_bv_call_pileup_device_on_reads_of_66000_bases(tmp_path):
    """`bv_call --pileup device` writes the default run's VCF and CVG around position 66,536"""
    from test_gpu_pileup_call import call
    exe = os.path.join(ROOT, "basevar_amd", "lib", "bv_call")
    assert os.path.exists(exe)
    fasta = str(tmp_path / "ref.fa")
    pr.write_fasta(fasta, rc.FA)
    bams = []
    for s, pos in enumerate((1000, 700)):
        header = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in pr.REFS) + "@RG\tID:x\tSM:smp%03d\n" % s
        bams.append(str(tmp_path / ("s%d.bam" % s)))
        bam_py.write_bam(bams[-1], pr.REFS, [rc.long_read(pos=pos, seed=66 + s)], header_text=header)
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", "chr1:66300-66700", "-q", str(pr.MAPQ_THD), "--thread", "2"]
    want = call(exe, args, "host", tmp_path)
    got = call(exe, args, "dev", tmp_path, ["--pileup", "device"])
    assert got[0] == want[0] and got[1] == want[1]
    assert want[1].count(b"\n") > 400 and got[2]["pileup"] == "device" and got[2]["sites"] == want[2]["sites"] == 401
