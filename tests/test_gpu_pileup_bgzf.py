"""GPU tests of bv_engine_pileup_bgzf (include/basevar_amd_pileup_bgzf.h): BAM files piled up from their compressed BGZF members.
The expectation is pileup() on the same engine from BamFile::next_raw's records -- a route the existing tests hold to the CPU
harness -- and pileup_bgzf() from the members that host/raw_members.hpp planned for the same fetches (inside
tests/cpp/bam_members_check.cpp, which has held the plan to next_raw on the CPU) must give the same planes, padding cells included,
the same depths, tokens, text and n_covered, byte for byte, and leave the engine in the same state for every call that follows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_members as bm  # noqa: E402
import bam_py  # noqa: E402
import pileup_ref as pr  # noqa: E402

N_MAX = 300
DATA = os.path.join(ROOT, "tests", "golden", "data")
CE_FASTA, CE_REF, CE_LEN = os.path.join(DATA, "ce.fa.gz"), "CHROMOSOME_I", 1009800


@pytest.fixture(scope="module")
def harness():
    return bm.build()


@pytest.fixture(scope="module")
def plans(harness, tmp_path_factory):
    """(corpus key, n samples, window) -> (corpus, Dump of the next_raw route, Plan, counts); corpora and plans made once"""
    tmp, corpora, cache = tmp_path_factory.mktemp("pileup_bgzf"), {}, {}

    def get(key, n, window):
        if key not in corpora:
            if key == "special":
                bams, fasta, fa = bm.write_special(tmp / "special")
                c = bm.Corpus.__new__(bm.Corpus)
                c.bams, c.fasta, c.fa = bams, fasta, fa
                corpora[key] = c
            else:
                bp, indexed, n_files, lead = key
                corpora[key] = bm.Corpus(tmp / ("c%d_%d_%d_%d" % key), n_files, bp, indexed, lead_empty=lead)
        c = corpora[key]
        if (key, n, window) not in cache:
            cache[(key, n, window)] = (c,) + bm.run_plan(harness, tmp / ("p%d.bin" % len(cache)), c.fasta, c.bams[:n], window)
        return cache[(key, n, window)]
    return get


BIG = (700, True, N_MAX, 0)  # 300 indexed files, 700 bytes a member


def engine(fa, max_sites=1024, n=N_MAX):
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=max_sites, min_af_value=bv.min_af(max(n, 1)), device=0, max_samples=max(n, 1))
    if fa is not None:
        e.pileup_set_reference(fa)
    return e


def state(eng, chrom):
    """everything the engine holds after a pileup: the fetched planes, depth, tokens, text, and the batchfile rows' text"""
    got = eng.pileup_fetch()
    off = eng.pileup_text(chrom)
    got["rows_off"], got["rows_text"] = off, eng.pileup_text_fetch()
    return got


def both(eng, d, p, n, window, region=pr.REGION, mapq=pr.MAPQ_THD, pitch=None, chrom=pr.REF_ID):
    """pileup() from the next_raw records, pileup_bgzf() from the planned members: the same engine state, and the harness's planes"""
    na = eng.pileup(d.records, d.run_off, d.run_sample, n, d.tid, region, window, mapq, pitch=pitch)
    a = state(eng, chrom)
    nb = eng.pileup_bgzf(p.data, p.member_off, p.runs, n, d.tid, region, window, mapq, pitch=pitch)
    b = state(eng, chrom)
    assert na == nb == d.n_covered
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    for f in ("cell", "qual", "mapq", "rank"):
        assert b[f][:, :n].tobytes() == getattr(d, f)[:, :n].tobytes(), f
    assert b["depth"].tobytes() == d.depth.tobytes() and b["tokens"].tobytes() == d.tokens.tobytes() and b["text"].tobytes() == d.text.tobytes()
    return b


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, N_MAX])
def test_planes_depths_tokens_text_are_pileups(plans, n):
    """1,000 rows at every sample count; pitch n rounded to 16 and a wider one"""
    c, d, p, counts = plans(BIG, n, pr.WINDOWS["w1000"])
    assert d.n_tokens > 0 and d.n_covered > 500 and counts["straddle"] > 0 and counts["begin_gt0"] > 0 and counts["end_lt_isize"] > 0
    eng = engine(c.fa)
    got = both(eng, d, p, n, pr.WINDOWS["w1000"])
    assert got["cell"].shape[1] == (n + 15) // 16 * 16
    both(eng, d, p, n, pr.WINDOWS["w1000"], pitch=(n + 15) // 16 * 16 + 48)
    eng.close()


@pytest.mark.parametrize("name", ["w1", "w2", "w64", "w65", "edge", "next"])
def test_small_windows_and_both_sides_of_the_steps_edge(plans, name):
    c, d, p, _ = plans(BIG, 65, pr.WINDOWS[name])
    eng = engine(c.fa)
    both(eng, d, p, 65, pr.WINDOWS[name])
    eng.close()


@pytest.mark.parametrize("bp", [100, 700, 60000])
@pytest.mark.parametrize("indexed", [False, True])
def test_member_sizes_with_and_without_an_index(plans, bp, indexed):
    """100 bytes a member: a 300-base record lies across three and more; 60,000: a file is one member and its end-of-file marker"""
    eng = None
    for name in ("w1000", "w65", "edge"):
        c, d, p, counts = plans((bp, indexed, 9, 0), 9, pr.WINDOWS[name])
        assert (counts["span3"] > 0) == (bp == 100) and (counts["straddle"] > 0) == (bp < 60000)
        assert (counts["isize0"] == 9) == (not indexed) and (counts["no_run"] == 1) == indexed
        eng = eng or engine(c.fa)
        both(eng, d, p, 9, pr.WINDOWS[name])
    eng.close()


def test_range_bam(harness, tmp_path):
    """the reference's own fixture with its index: windows with reads, without reads and without a chunk"""
    eng = engine(bam_py.read_fasta(CE_FASTA, CE_REF), n=2)
    for w, runs, covered in (((900, 1200), 2, 207), ((1000, 1063), 2, None), ((1, 64), 2, 0), ((20000, 20100), 0, 0)):
        d, p, counts = bm.run_plan(harness, tmp_path / "r.bin", CE_FASTA, [bm.RANGE_BAM, bm.RANGE_BAM], w, ref_id=CE_REF, region=(1, CE_LEN), mapq_thd=10)
        assert counts["runs"] == runs and (covered is None or d.n_covered == covered)
        both(eng, d, p, 2, w, region=(1, CE_LEN), mapq=10, chrom=CE_REF)
    eng.close()


def test_two_runs_that_share_a_member(plans):
    """two chunks of one fetch meet inside one member: the member is handed over once and both runs are cut from it"""
    for w in (bm.SHARED_WINDOW, (bm.SHARED_WINDOW[0], bm.SHARED_WINDOW[0])):
        c, d, p, counts = plans("special", 3, w)
        assert counts["shared"] == 2 and counts["multi_run"] == 2 and counts["chunk_end_low0"] >= 1
        r = p.runs
        assert any(r["sample"][k] == r["sample"][k - 1] and r["first_member"][k] == r["first_member"][k - 1] + r["n_members"][k - 1] - 1 for k in range(1, len(r)))
        eng = engine(c.fa, n=3)
        both(eng, d, p, 3, w)
        eng.close()


def test_leading_samples_without_a_run(plans):
    key = (700, True, 20, 3)
    c, d, p, counts = plans(key, 20, pr.WINDOWS["w1000"])
    assert int(p.runs["sample"].min()) >= 3 and counts["no_run"] >= 4
    eng = engine(c.fa)
    both(eng, d, p, 20, pr.WINDOWS["w1000"])
    # ... and a cohort that is only such samples: no run at all, no member at all
    c, d, p, counts = plans(key, 3, pr.WINDOWS["w64"])
    assert counts["runs"] == 0 and counts["members"] == 0
    got = both(eng, d, p, 3, pr.WINDOWS["w64"])
    assert (got["cell"] == 8).all() and not got["rank"].any() and not got["depth"].any()
    eng.close()


@pytest.mark.parametrize("tagged", [False, True])
def test_rows_and_submit_behind_it(plans, tagged):
    """pileup_rows + bv_engine_submit behind pileup_bgzf give what they give behind pileup(): lrt_pileup_bgzf equals lrt_pileup"""
    c, d, p, _ = plans(BIG, 65, pr.WINDOWS["w1000"])
    eng = engine(c.fa)
    w = pr.WINDOWS["w1000"]
    a = eng.lrt_pileup(d.records, d.run_off, d.run_sample, 65, d.tid, pr.REGION, w, pr.MAPQ_THD, tagged=tagged)
    b = eng.lrt_pileup_bgzf(p.data, p.member_off, p.runs, 65, d.tid, pr.REGION, w, pr.MAPQ_THD, tagged=tagged)
    assert len(a.sites) == d.n_covered > 500 and a.n_variant == b.n_variant > 0
    assert a.sites.tobytes() == b.sites.tobytes() and a.positions.tobytes() == b.positions.tobytes() and a.depth.tobytes() == b.depth.tobytes()
    assert a.tokens == b.tokens and len(a.tokens) == d.n_tokens
    eng.close()


def test_calls_in_either_order_give_their_own_results(plans):
    """pileup() right behind pileup_bgzf() and the other way round, on windows and cohorts of different sizes: no stale buffer"""
    c, d1, p1, _ = plans(BIG, 65, pr.WINDOWS["w1000"])
    _, d2, p2, _ = plans(BIG, 2, pr.WINDOWS["w64"])
    eng = engine(c.fa)

    def check(got, d, n):
        for f in ("cell", "qual", "mapq", "rank"):
            assert got[f][:, :n].tobytes() == getattr(d, f)[:, :n].tobytes(), f
            assert (got[f][:, n:] == (8 if f == "cell" else 0)).all()
        assert got["depth"].tobytes() == d.depth.tobytes() and got["tokens"].tobytes() == d.tokens.tobytes() and got["text"].tobytes() == d.text.tobytes()

    args = lambda n, name: (n, 1, pr.REGION, pr.WINDOWS[name], pr.MAPQ_THD)
    eng.pileup_bgzf(p1.data, p1.member_off, p1.runs, *args(65, "w1000")); check(eng.pileup_fetch(), d1, 65)
    eng.pileup(d2.records, d2.run_off, d2.run_sample, *args(2, "w64")); check(eng.pileup_fetch(), d2, 2)
    eng.pileup_bgzf(p2.data, p2.member_off, p2.runs, *args(2, "w64")); check(eng.pileup_fetch(), d2, 2)
    eng.pileup(d1.records, d1.run_off, d1.run_sample, *args(65, "w1000")); check(eng.pileup_fetch(), d1, 65)
    eng.pileup_bgzf(p2.data, p2.member_off, p2.runs, *args(2, "w64")); check(eng.pileup_fetch(), d2, 2)
    eng.pileup_bgzf(p1.data, p1.member_off, p1.runs, *args(65, "w1000")); check(eng.pileup_fetch(), d1, 65)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------- refusals
def call(eng, p, n=9, window=pr.WINDOWS["w1000"], region=pr.REGION, tid=pr.TID, pitch=16, runs=None, member_off=None, data=None, edit=None, n_covered=True):
    """bv_engine_pileup_bgzf as C callers see it: (status, message)"""
    from basevar_amd import _capi
    data = p.data if data is None else data
    off = np.ascontiguousarray(p.member_off if member_off is None else member_off, np.uint64)
    runs = np.ascontiguousarray(p.runs if runs is None else runs)
    a = _capi.PileupBgzf()
    a.members = _capi.BgzfMembers(data.ctypes.data, off.ctypes.data, int(data.size), int(off.size) - 1, 0)
    a.runs, a.pitch, a.n_runs, a.n_samples, a.tid = runs.ctypes.data, pitch, int(runs.size), n, tid
    a.region_beg, a.region_end, a.beg, a.end, a.mapq_thd = region[0], region[1], window[0], window[1], pr.MAPQ_THD
    if edit:
        edit(a)
    n_cov = C.c_uint32(0)
    rc = eng._lib.bv_engine_pileup_bgzf(eng._h, C.byref(a), C.byref(n_cov) if n_covered else None, None)
    return rc, eng._err()


def test_refusals_come_from_the_host_bytes_and_leave_the_engine_usable(plans):
    from basevar_amd import _capi
    c, d, p, _ = plans((700, True, 9, 0), 9, pr.WINDOWS["w1000"])
    eng = engine(c.fa)
    r0 = p.runs
    last = r0["first_member"] + r0["n_members"] - 1
    multi = int(np.flatnonzero(r0["n_members"] > 1)[0])

    def runs_with(k, **kw):
        r = r0.copy()
        for f, v in kw.items():
            r[f][k] = v
        return r

    def setter(**kw):
        def edit(a):
            for f, v in kw.items():
                setattr(a, f, v)
        return edit

    def members_reserved(a):
        a.members.reserved_ = 1

    def null_data(a):
        a.members.data = None

    def null_off(a):
        a.members.member_off = None

    off_bad = p.member_off.copy(); off_bad[2] = off_bad[1] - 1
    off_short = p.member_off.copy(); off_short[2] = off_short[1] + 25
    invalid = {
        "reserved_": dict(edit=setter(reserved_=1)),
        "members.reserved_": dict(edit=members_reserved),
        "a run's reserved_": dict(runs=runs_with(1, reserved_=7)),
        "pitch no multiple of 16": dict(pitch=24),
        "pitch below n_samples": dict(n=17, pitch=16),
        "no sample": dict(n=0),
        "negative tid": dict(tid=-1),
        "window across the step grid": dict(window=(499990, 500010)),
        "window outside the region": dict(window=(1000, 1999), region=(1500, 600000)),
        "window beyond the reference": dict(window=(600001, 600010), region=(1, 700000)),
        "null n_covered": dict(n_covered=False),
        "null runs": dict(edit=setter(runs=None)),
        "null data": dict(edit=null_data),
        "null member_off": dict(edit=null_off),
        "member_off out of order": dict(member_off=off_bad),
        "a member below 26 bytes": dict(member_off=off_short),
        "member_off beyond data_bytes": dict(data=p.data[:-1].copy()),
        "sample descends": dict(runs=runs_with(2, sample=0)),
        "sample beyond n_samples": dict(runs=runs_with(len(r0) - 1, sample=9)),
        "no member in a run": dict(runs=runs_with(1, n_members=0)),
        "members beyond n_members": dict(runs=runs_with(len(r0) - 1, n_members=int(r0["n_members"][-1]) + 1)),
        "first_member beyond n_members": dict(runs=runs_with(1, first_member=0xFFFFFFFF, n_members=2)),
        "begin above ISIZE": dict(runs=runs_with(multi, begin=int(p.isize[r0["first_member"][multi]]) + 1)),
        "end above ISIZE": dict(runs=runs_with(multi, end=int(p.isize[last[multi]]) + 1)),
        "begin above end in one member": dict(runs=runs_with(multi, n_members=1, begin=10, end=9)),
    }
    for what, kw in invalid.items():
        rc, msg = call(eng, p, **kw)
        assert rc == _capi.BV_ERR_INVALID_ARG and "bv_engine_pileup_bgzf" in msg, (what, rc, msg)
        with pytest.raises(RuntimeError):  # ... and the engine holds no pileup
            eng.pileup_fetch()
    rc, msg = call(eng, p, window=(1, 500001))
    assert rc == _capi.BV_ERR_TOO_LARGE and "bv_pileup_max_rows" in msg
    fresh = engine(None)
    rc, msg = call(fresh, p)
    assert rc == _capi.BV_ERR_INVALID_ARG and "no reference set" in msg
    fresh.close()
    rc, msg = call(eng, p)  # the unedited call is good
    assert rc == 0
    both(eng, d, p, 9, pr.WINDOWS["w1000"])
    eng.close()


def test_no_run_is_ok_and_every_cell_unclaimed():
    eng = engine("ACGT" * 1000, n=5)
    n_cov = eng.pileup_bgzf(b"", [0], np.zeros(0, bm.RUN_DTYPE), 5, 0, (1, 4000), (100, 163), 10)
    got = eng.pileup_fetch()
    assert n_cov == 0 and got["cell"].shape == (64, 16) and (got["cell"] == 8).all() and not got["rank"].any() and not got["depth"].any()
    eng.close()


def test_damaged_members_and_cut_points_are_data_errors(plans):
    """statuses, not faults: a refused call names what is damaged, the engine holds no pileup, and a good call follows"""
    from basevar_amd import _capi
    c, d, p, _ = plans((700, True, 9, 0), 9, pr.WINDOWS["w1000"])
    eng = engine(c.fa)
    r0 = p.runs
    run = int(np.flatnonzero(r0["n_members"] > 2)[1])  # not the first run, a member in its middle
    k = int(r0["first_member"][run]) + 1
    assert p.isize[k] > 0
    for what, at in (("payload", int(p.member_off[k]) + 18 + 7), ("crc", int(p.member_off[k + 1]) - 8)):
        data = p.data.copy()
        data[at] ^= 0x40
        rc, msg = call(eng, p, data=data)
        assert rc == _capi.BV_ERR_DATA and "member %d " % k in msg and "sample %d, run %d" % (int(r0["sample"][run]), run) in msg, (what, rc, msg)
        assert what != "crc" or "status 4" in msg
        with pytest.raises(RuntimeError):
            eng.pileup_fetch()
        both(eng, d, p, 9, pr.WINDOWS["w1000"])
    # an end inside the first record of a sample's first run (a damaged index): the record overruns its run
    runs = r0.copy()
    assert runs["sample"][run] != runs["sample"][run - 1] and int(runs["begin"][run]) + 10 <= int(p.isize[runs["first_member"][run]])
    runs["n_members"][run], runs["end"][run] = 1, int(runs["begin"][run]) + 10
    rc, msg = call(eng, p, runs=runs)
    assert rc == _capi.BV_ERR_DATA and "sample %d, run %d, the record at byte 0 of the run" % (int(r0["sample"][run]), run) in msg and "overruns its run" in msg, msg
    with pytest.raises(RuntimeError):
        eng.pileup_fetch()
    both(eng, d, p, 9, pr.WINDOWS["w1000"])
    eng.close()
