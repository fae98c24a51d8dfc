"""GPU tests of `bv_pileup --rows device` (the samples' raw BAM records piled up on an engine, the rows written where the planes lie
and, for a `.gz` output, deflated there: bv_engine_pileup / _pileup_text / _pileup_text_deflate) against `bv_pileup` without the
flag: `.gz` outputs inflate to identical bytes, plain outputs are identical files -- whatever --window, --rows-per-call and
--deflate-level say --, and `bv_call --batchfiles` gives the same VCF and CVG from either file."""
import gzip
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pileup_ref as pr  # noqa: E402
from test_gpu_pileup_call import cohort  # noqa: E402

BV_PILEUP = os.path.join(ROOT, "basevar_amd", "lib", "bv_pileup")
BV_CALL = os.path.join(ROOT, "basevar_amd", "lib", "bv_call")


@pytest.fixture(scope="module")
def tools():
    import __graft_entry__ as g
    if not (os.path.exists(BV_PILEUP) and os.path.exists(BV_CALL)):
        g.build()
    return BV_PILEUP, BV_CALL


@pytest.fixture(scope="module", params=[3, 130])
def cohort_n(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("ptext_cohort_%d" % request.param)
    return (request.param,) + cohort(d, request.param)


def pileup(exe, fasta, bams, region, out, extra=()):
    args = [exe, "-R", fasta, "--regions", region, "-q", str(pr.MAPQ_THD), "--thread", "4", "-o", str(out)] + sum((["-I", b] for b in bams), []) + list(extra)
    p = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return open(str(out), "rb").read()


REGION = "chr1:900-2300"
VARIANTS = {"default": [], "window_64_rows_per_call_7": ["--window", "64", "--rows-per-call", "7"], "small": ["--deflate-level", "small"],
            "small_window_64_rows_per_call_7": ["--deflate-level", "small", "--window", "64", "--rows-per-call", "7"], "rows_per_call_1": ["--rows-per-call", "1"]}


@pytest.fixture(scope="module")
def host_files(tools, cohort_n, tmp_path_factory):
    """the default route's `.gz` and plain batchfile of the cohort, written once"""
    n, fasta, bams, ids = cohort_n
    d = tmp_path_factory.mktemp("ptext_host_%d" % n)
    want_gz = pileup(tools[0], fasta, bams, REGION, d / "host.bf.gz")
    want = pileup(tools[0], fasta, bams, REGION, d / "host.bf")
    assert gzip.decompress(want_gz) == want and want.count(b"\n") > 1401 and want.count(b"+") > 100 * min(n, 50)
    return want_gz, want


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_rows_device_writes_the_default_routes_batchfile(tools, cohort_n, host_files, tmp_path, variant):
    n, fasta, bams, ids = cohort_n
    want_gz, want = host_files
    extra = VARIANTS[variant]
    got_gz = pileup(tools[0], fasta, bams, REGION, tmp_path / "dev.bf.gz", ["--rows", "device"] + extra)
    assert gzip.decompress(got_gz) == want
    assert got_gz[-28:] == want_gz[-28:]  # the end-of-file member
    if "small" not in variant:
        assert pileup(tools[0], fasta, bams, REGION, tmp_path / "dev.bf", ["--rows", "device"] + extra) == want


def test_rows_device_across_the_step_edge(tools, cohort_n, tmp_path):
    n, fasta, bams, ids = cohort_n
    region = "chr1:499900-500100"
    want = pileup(tools[0], fasta, bams, region, tmp_path / "host.bf")
    assert pileup(tools[0], fasta, bams, region, tmp_path / "dev.bf", ["--rows", "device"]) == want
    assert gzip.decompress(pileup(tools[0], fasta, bams, region, tmp_path / "dev.bf.gz", ["--rows", "device", "--window", "64", "--rows-per-call", "7"])) == want
    # a region no read covers: every row is placeholders, and is written
    region = "chr1:300000-300070"
    want = pileup(tools[0], fasta, bams, region, tmp_path / "none.bf")
    assert want.count(b"\n") > 71 and pileup(tools[0], fasta, bams, region, tmp_path / "none_dev.bf", ["--rows", "device"]) == want


def test_bv_call_reads_either_batchfile_alike(tools, cohort_n, tmp_path):
    n, fasta, bams, ids = cohort_n
    # (the rows behind 1800 hold the indels of the corpus's empty reads: their quality, 255, is written as the byte 0x20, a row
    # that no batchfile reader takes, whichever route wrote it)
    region = "chr1:900-1800"
    pileup(tools[0], fasta, bams, region, tmp_path / "host.bf.gz")
    pileup(tools[0], fasta, bams, region, tmp_path / "dev.bf.gz", ["--rows", "device"])
    outs = []
    for tag in ("host", "dev"):
        v, c = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".cvg"))
        p = subprocess.run([tools[1], "--batchfiles", str(tmp_path / (tag + ".bf.gz")), "--output-vcf", v, "--output-cvg", c], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append((open(v, "rb").read(), open(c, "rb").read()))
    assert outs[0] == outs[1] and outs[0][1].count(b"\n") > 600


def test_bam_files_that_number_the_contig_differently_are_refused(tools, tmp_path):
    import bam_py
    import numpy as np
    fa = pr.reference()
    fasta = str(tmp_path / "ref.fa")
    pr.write_fasta(fasta, fa)
    rng = np.random.default_rng(1)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    head = lambda refs, s: "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "@RG\tID:x\tSM:%s\n" % s
    bam_py.write_bam(a, pr.REFS, [pr.read(rng, 1100, [(pr.M, 40)])], header_text=head(pr.REFS, "sa"))
    other = [pr.REFS[1], pr.REFS[0], pr.REFS[2]]
    bam_py.write_bam(b, other, [pr.read(rng, 1100, [(pr.M, 40)], tid=0)], header_text=head(other, "sb"))
    want = pileup(tools[0], fasta, [a, b], "chr1:1000-1200", tmp_path / "host.bf")
    assert want.count(b"\n") > 200
    p = subprocess.run([tools[0], "-R", fasta, "--regions", "chr1:1000-1200", "-o", str(tmp_path / "dev.bf"), "-I", a, "-I", b, "--rows", "device"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 1 and "needs BAM files that number chr1 alike: " + b in p.stderr
