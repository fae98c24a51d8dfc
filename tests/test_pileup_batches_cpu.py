"""CPU tests (no GPU) of `bv_pileup -B N` on the default route (--rows host): the reference's batches (_create_batchfiles,
src/basetype_caller.cpp:427-442) -- the samples in input order cut into ceil(n / N) batches, batch j written to
PREFIX.<j>_<bn>.bf.gz with a header of its own -- and every file inflates to the bytes of a `bv_pileup` run without -B over that
slice of the samples."""
import glob
import gzip
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pileup_ref as pr  # noqa: E402
from test_gpu_pileup_call import cohort  # noqa: E402

BV_PILEUP = os.path.join(ROOT, "basevar_amd", "lib", "bv_pileup")
REGION = "chr1:900-2300"
N_COHORT = 130


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as g
    g.build()
    return BV_PILEUP


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    return cohort(tmp_path_factory.mktemp("batches_cohort"), N_COHORT)


def run(exe, fasta, bams, out, extra=(), region=REGION):
    args = [exe, "-R", fasta, "--regions", region, "-q", str(pr.MAPQ_THD), "--thread", "4", "-o", str(out)] + sum((["-I", b] for b in bams), []) + list(extra)
    p = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p


def batch_names(prefix, n, b, ext=".bf.gz"):
    bn = (n + b - 1) // b
    return ["%s.%d_%d%s" % (prefix, j, bn, ext) for j in range(1, bn + 1)]


@pytest.fixture(scope="module")
def slices(exe, samples, tmp_path_factory):
    """the batchfile of a run without -B over samples [lo, hi), written once a slice"""
    fasta, bams, ids = samples
    d = tmp_path_factory.mktemp("batches_slices")
    done = {}

    def get(lo, hi):
        if (lo, hi) not in done:
            out = d / ("s%d_%d.bf" % (lo, hi))
            run(exe, fasta, bams[lo:hi], out)
            done[(lo, hi)] = open(str(out), "rb").read()
        return done[(lo, hi)]

    return get


@pytest.mark.parametrize("b,n", [(1, 5), (7, N_COHORT), (64, N_COHORT), (130, N_COHORT), (200, N_COHORT)])
def test_batch_count_writes_the_references_files(exe, samples, slices, tmp_path, b, n):
    fasta, bams, ids = samples
    prefix = str(tmp_path / "cohort")
    p = run(exe, fasta, bams[:n], prefix, ["-B", str(b), "--rows", "host"])
    names = batch_names(prefix, n, b)
    assert sorted(glob.glob(prefix + "*")) == sorted(names)  # the reference's names, and nothing else
    if b >= n:
        assert names == [prefix + ".1_1.bf.gz"]
    assert "%d batchfiles of %d samples" % (len(names), b) in p.stderr and "passes" not in p.stderr
    sizes = []
    for j, name in enumerate(names):
        lo, hi = j * b, min(n, (j + 1) * b)
        got = gzip.decompress(open(name, "rb").read())
        assert got == slices(lo, hi), name
        head = got.split(b"\n", 2)
        assert head[0] == b"##fileformat=BaseVarBatchFile_v1.0" and head[1] == b"##SampleIDs=" + ",".join(ids[lo:hi]).encode()
        assert got.count(b"\n") > 1401
        sizes.append(hi - lo)
    assert sum(sizes) == n and all(x == b for x in sizes[:-1]) and 0 < sizes[-1] <= b
    if n % b and b < n:
        assert sizes[-1] == n % b < b  # the remainder batch is smaller


def test_output_plain_and_the_long_option(exe, samples, slices, tmp_path):
    fasta, bams, ids = samples
    prefix = str(tmp_path / "plain")
    run(exe, fasta, bams[:20], prefix, ["--batch-count", "7", "--output-plain"])
    names = batch_names(prefix, 20, 7, ".bf")
    assert sorted(glob.glob(prefix + "*")) == sorted(names) and len(names) == 3
    for j, name in enumerate(names):
        assert open(name, "rb").read() == slices(j * 7, min(20, (j + 1) * 7))
    # a PREFIX that ends in .gz is taken as it is
    prefix = str(tmp_path / "odd.gz")
    run(exe, fasta, bams[:3], prefix, ["-B", "2"])
    assert sorted(glob.glob(prefix + "*")) == [prefix + ".1_2.bf.gz", prefix + ".2_2.bf.gz"]
    assert gzip.decompress(open(prefix + ".2_2.bf.gz", "rb").read()) == slices(2, 3)


def test_without_batch_count_the_tool_is_what_it_was(exe, samples, slices, tmp_path):
    fasta, bams, ids = samples
    out = tmp_path / "one.bf.gz"
    p = run(exe, fasta, bams[:5], out)
    assert gzip.decompress(open(str(out), "rb").read()) == slices(0, 5)
    assert p.stderr.strip() == "[INFO] %s: 5 samples, chr1:900-2300" % out
    q = subprocess.run([exe, "-R", fasta, "--regions", REGION, "-o", str(tmp_path / "x"), "-I", bams[0], "-B", "0"], capture_output=True, text=True)
    assert q.returncode == 1 and "--batch-count wants a number >= 1" in q.stderr
