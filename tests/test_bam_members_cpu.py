"""CPU tests (no GPU) of the host planner behind bv_engine_pileup_bgzf, basevar_amd/host/raw_members.hpp: a window's fetches as
whole compressed BGZF members plus cut points, nothing inflated.  The stand-alone harness tests/cpp/bam_members_check.cpp (built
with ASan + UBSan and run as a program) plans every file and window below, inflates the planned members with zlib, cuts the runs,
requires that every run is a chain of whole records that ends exactly at the run's end, and requires that bv_pileup_core.h's pileup
over the runs gives the planes, depths and tokens of the core over BamFile::next_raw's bytes of the same fetch, byte for byte.  That
the corpus reaches the cases a planner can get wrong is asserted from the plans.  Also: the new header against the ctypes layer,
and bv_pileup's refusal of --inflate device in a build without the device route."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_members as bm  # noqa: E402
import bam_py  # noqa: E402
import bai_py  # noqa: E402
import pileup_ref as pr  # noqa: E402

N_SAMPLES = 9
DATA = os.path.join(ROOT, "tests", "golden", "data")
CE_FASTA, CE_REF, CE_LEN = os.path.join(DATA, "ce.fa.gz"), "CHROMOSOME_I", 1009800
RANGE_WINDOWS = [(900, 1200), (1000, 1063), (1500, 1600), (1, 64), (20000, 20100), (CE_LEN - 63, CE_LEN)]  # the last three: no read; two: no chunk
CORPORA = [(100, False), (700, False), (60000, False), (100, True), (700, True), (60000, True)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from basevar_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def harness(lib):
    return bm.build(asan=True)


@pytest.fixture(scope="module")
def plans(harness, tmp_path_factory):
    """every (file set, window) through the harness under the sanitizers, once: {name: (Dump, Plan, counts)}"""
    tmp = tmp_path_factory.mktemp("bam_members")
    out = {}
    for w in RANGE_WINDOWS:
        out["range_%d" % w[0]] = bm.run_plan(harness, tmp / "r.bin", CE_FASTA, [bm.RANGE_BAM, bm.RANGE_BAM], w, ref_id=CE_REF, region=(1, CE_LEN), mapq_thd=10)
    for bp, indexed in CORPORA:
        c = bm.Corpus(tmp / ("c%d_%d" % (bp, indexed)), N_SAMPLES, bp, indexed)
        for name in sorted(pr.WINDOWS):
            out["corpus_%d_%d_%s" % (bp, indexed, name)] = bm.run_plan(harness, tmp / "c.bin", c.fasta, c.bams, pr.WINDOWS[name])
    bams, fasta, _ = bm.write_special(tmp / "special")
    for w in (bm.SHARED_WINDOW, (bm.SHARED_WINDOW[0], bm.SHARED_WINDOW[0]), (1000, 1063)):
        out["special_%d_%d" % w] = bm.run_plan(harness, tmp / "s.bin", fasta, bams, w)
    return out


def test_every_plan_piles_up_to_next_raws_result(plans):
    """(run_plan raises when the harness exits non-zero: a run that is no chain of whole records, planes that differ, a report)"""
    assert len(plans) == len(RANGE_WINDOWS) + len(CORPORA) * len(pr.WINDOWS) + 3
    for name, (d, p, counts) in plans.items():
        assert d.status == 0, name
        assert counts["members"] == len(p.member_off) - 1 and counts["runs"] == len(p.runs), name
    assert plans["range_900"][0].n_covered == 207  # the reference's own test command: 207 covered rows
    assert plans["corpus_700_1_w1000"][0].n_covered == 1000 and plans["corpus_700_1_w1000"][0].n_tokens > 0


def test_plans_are_what_the_engine_takes(plans):
    """the runs' fields as include/basevar_amd_pileup_bgzf.h states them, from the dumped plans alone"""
    for name, (d, p, _) in plans.items():
        n = len(p.member_off) - 1
        r = p.runs
        assert (np.diff(p.member_off.astype(np.int64)) >= 26).all() and int(p.member_off[-1]) == p.data.size, name
        if not len(r):
            assert p.tid == -1
            continue
        last = r["first_member"] + r["n_members"] - 1
        assert (r["n_members"] >= 1).all() and (last < n).all() and not r["reserved_"].any(), name
        assert (np.diff(r["sample"].astype(np.int64)) >= 0).all() and (r["begin"] <= p.isize[r["first_member"]]).all() and (r["end"] <= p.isize[last]).all(), name
        one = r["n_members"] == 1
        assert (r["begin"][one] <= r["end"][one]).all(), name
        assert (np.diff(r["first_member"].astype(np.int64)) >= 0).all(), name  # no member is read twice: a later run starts at or behind the last member so far
        assert p.tid == d.tid


def test_the_corpus_reaches_what_a_planner_can_get_wrong(plans):
    """asserted from the plans, not from how the files were built"""
    total = {k: sum(c[k] for _, _, c in plans.values()) for k in bm.COUNTS}
    for k in ("begin_gt0", "end_lt_isize", "chunk_end_low0", "straddle", "span3", "multi_run", "shared", "no_run", "isize0"):
        assert total[k] >= 1, (k, total)
    # ... and where: records over three members only at 100 bytes a member, shared members in the file built for them, a
    # begin of zero too (range.bam's records start their member)
    assert all(c["span3"] == 0 for n, (_, _, c) in plans.items() if not n.startswith("corpus_100_"))
    assert plans["special_%d_%d" % bm.SHARED_WINDOW][2]["shared"] == 2 and plans["special_%d_%d" % bm.SHARED_WINDOW][2]["chunk_end_low0"] >= 1
    assert any(len(p.runs) and (p.runs["begin"] == 0).any() for _, p, _ in plans.values())
    assert plans["range_20000"][2]["runs"] == 0 and plans["range_20000"][2]["no_run"] == 2  # a window with no chunk
    # an unindexed file is one run to the last member before the end of the file, the empty end-of-file member included
    d, p, c = plans["corpus_700_0_w64"]
    assert c["runs"] == N_SAMPLES and c["isize0"] == N_SAMPLES and (p.runs["end"] == 0).all()


def test_bai_py_writes_what_the_reader_and_the_spec_say(tmp_path):
    """bai_py against bam_py.reg2bins (a record's bin is among the bins of its own span) and the fetch of every window through it
    against the scan of the file without an index (inside the harness: next_raw over the chunks gives the scan's planes)"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        beg = int(rng.integers(0, 1 << 28))
        end = beg + int(rng.choice([1, 2, 100, 1 << 14, 1 << 17, 1 << 22]))
        assert bai_py.reg2bin(beg, end) in bam_py.reg2bins(beg, end)
    assert bai_py.reg2bin(0, 1 << 14) == 4681 and bai_py.reg2bin(0, (1 << 14) + 1) == 585 and bai_py.reg2bin((1 << 14) - 1, (1 << 14) + 1) == 585


def test_indexed_and_unindexed_files_pile_up_alike(plans):
    for bp in (100, 700, 60000):
        for name in pr.WINDOWS:
            a, b = plans["corpus_%d_0_%s" % (bp, name)][0], plans["corpus_%d_1_%s" % (bp, name)][0]
            for f in ("cell", "qual", "mapq", "rank", "depth", "tokens", "text"):
                assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (bp, name, f)


def test_a_member_of_another_packing_is_an_error_that_names_file_and_offset(harness, tmp_path):
    """a later member with a longer extra field (valid BGZF, not the XLEN = 6 packing): the planner refuses, the host reader reads it"""
    c = bm.Corpus(tmp_path / "c", 1, 700, False)
    blocks = bam_py.bgzf_blocks(c.bams[0])
    raw = open(c.bams[0], "rb").read()
    off, total, _ = blocks[2]
    m = raw[off:off + total]
    wide = m[:10] + (10).to_bytes(2, "little") + m[12:16] + (total + 4 - 1).to_bytes(2, "little") + b"XY\0\0" + m[18:]
    with open(c.bams[0], "wb") as f:
        f.write(raw[:off] + wide + raw[off + total:])
    with pytest.raises(RuntimeError) as e:
        bm.run_plan(harness, tmp_path / "o.bin", c.fasta, c.bams, pr.WINDOWS["w64"])
    assert "s000.bam" in str(e.value) and "offset %d" % off in str(e.value) and "XLEN = 6" in str(e.value)


# ---------------------------------------------------------------------------------------------------------- the header
def test_pileup_bgzf_header_symbols_are_bound_and_exported(lib):
    from basevar_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "basevar_amd_pileup_bgzf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(bv_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.PILEUP_BGZF_EXPORTS) == ["bv_engine_pileup_bgzf"]
    assert not set(names) & (set(_capi.EXPORTS) | set(_capi.BGZF_EXPORTS) | set(_capi.VCF_EXPORTS) | set(_capi.PILEUP_EXPORTS) | set(_capi.PILEUP_TEXT_EXPORTS))
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bv_engine_pileup_bgzf(None, None, None, None) == _capi.BV_ERR_INVALID_ARG and b"null engine" in lib.bv_last_error(None)


def test_pileup_bgzf_struct_layouts_match_header(lib, tmp_path):
    from basevar_amd import _capi
    structs = [("bv_pileup_bgzf_run", _capi.PileupBgzfRun), ("bv_pileup_bgzf", _capi.PileupBgzf), ("bv_bgzf_members", _capi.BgzfMembers)]
    body = "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (n, f, n, f) for n, t in structs for f, _ in t._fields_)
    body += "".join('printf("%s.sizeof %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in structs)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "basevar_amd_pileup_bgzf.h"\nint main(void){\n' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = dict((a, int(b)) for a, b in (l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines()))
    for n, t in structs:
        assert vals[n + ".sizeof"] == C.sizeof(t)
        for f, _ in t._fields_:
            assert vals["%s.%s" % (n, f)] == getattr(t, f).offset, (n, f)
    assert vals["bv_pileup_bgzf_run.sizeof"] == _capi.PILEUP_BGZF_RUN_DTYPE.itemsize == bm.RUN_DTYPE.itemsize == 24
    for f in bm.RUN_DTYPE.names:
        assert vals["bv_pileup_bgzf_run." + f] == _capi.PILEUP_BGZF_RUN_DTYPE.fields[f][1] == bm.RUN_DTYPE.fields[f][1]


def test_kernel_counts_stand(lib):
    """the new entry adds no kernel of the pinned families: four bv_pileup_ kernels, one inflate kernel"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_scratch", os.path.join(ROOT, "tools", "kernel_scratch.py"))
    ks_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks_mod)
    if not os.path.exists(ks_mod.READELF):
        pytest.skip("llvm-readelf not found")
    from basevar_amd import _capi
    ks = ks_mod.kernels(_capi.LIB_PATH)
    assert len([k for k in ks if "bv_pileup_" in k["name"]]) == 4 and len([k for k in ks if "bv_bgzf_inflate_kernel" in k["name"]]) == 1


def test_bv_pileup_without_the_device_route_refuses_inflate_device(lib, tmp_path):
    """the sanitize build of bv_pileup has no device route: --inflate device is refused with a message, nothing is written"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "basevar_amd", "csrc"), "../lib/san/bv_pileup.asan"])
    tool = os.path.join(ROOT, "basevar_amd", "lib", "san", "bv_pileup.asan")
    out = tmp_path / "o.bf.gz"
    p = subprocess.run([tool, "-R", CE_FASTA, "--regions", "%s:900-1200" % CE_REF, "--mapq", "10", "-o", str(out), "-I", bm.RANGE_BAM, "--rows", "device", "--inflate", "device"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--inflate device" in p.stderr and not out.exists()
    p = subprocess.run([tool, "-R", CE_FASTA, "--regions", "%s:900-1200" % CE_REF, "--mapq", "10", "-o", str(out), "-I", bm.RANGE_BAM, "--inflate", "sideways"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--inflate" in p.stderr
