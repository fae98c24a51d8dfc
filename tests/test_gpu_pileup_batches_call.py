"""GPU tests of `bv_pileup --rows device -B N` (one engine for the run; --batches-per-pass K batches piled up as one wide pileup and
written as K sample parts of it: bv_engine_pileup[_bgzf] / _pileup_text_parts / _pileup_text_deflate with blocks cut at the parts)
against `bv_pileup --rows host -B N`: every file inflates to the same bytes -- whatever --batches-per-pass, --inflate,
--deflate-level and --rows-per-call say, also across the 500 kb step edge --, and `bv_call --batchfiles` on the files gives the VCF
and CVG of the single whole-cohort batchfile."""
import gzip
import itertools
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pileup_ref as pr  # noqa: E402
from test_gpu_pileup_call import cohort  # noqa: E402
from test_pileup_batches_cpu import batch_names  # noqa: E402

BV_PILEUP = os.path.join(ROOT, "basevar_amd", "lib", "bv_pileup")
BV_CALL = os.path.join(ROOT, "basevar_amd", "lib", "bv_call")
REGION = "chr1:1000-1200"
EDGE = "chr1:499900-500100"
# (cohort, N): N = 1 on the 3-sample cohort; 200 exceeds the 130 samples and gives one file
BATCHES = [(3, 1), (130, 7), (130, 64), (130, 200)]
PER_PASS = [1, 3, 0]  # 0: all batches in one pass
VARIANTS = list(itertools.product(("host", "device"), ("fast", "small"), (1, 0)))  # --inflate, --deflate-level, --rows-per-call (0: default)


@pytest.fixture(scope="module")
def tools():
    import __graft_entry__ as g
    if not (os.path.exists(BV_PILEUP) and os.path.exists(BV_CALL)):
        g.build()
    return BV_PILEUP, BV_CALL


@pytest.fixture(scope="module")
def cohorts(tmp_path_factory):
    made = {}

    def get(n):
        if n not in made:
            made[n] = cohort(tmp_path_factory.mktemp("batches_cohort_%d" % n), n)
        return made[n]

    return get


def pileup(exe, fasta, bams, region, out, extra=()):
    args = [exe, "-R", fasta, "--regions", region, "-q", str(pr.MAPQ_THD), "--thread", "4", "-o", str(out)] + sum((["-I", b] for b in bams), []) + list(extra)
    p = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p


@pytest.fixture(scope="module")
def host_files(tools, cohorts, tmp_path_factory):
    """the inflated files of `--rows host -B N`, written once per (cohort, N, region)"""
    done = {}

    def get(n, b, region):
        if (n, b, region) not in done:
            fasta, bams, ids = cohorts(n)
            prefix = str(tmp_path_factory.mktemp("batches_host") / "h")
            pileup(tools[0], fasta, bams, region, prefix, ["-B", str(b), "--rows", "host"])
            done[(n, b, region)] = [gzip.decompress(open(f, "rb").read()) for f in batch_names(prefix, n, b)]
        return done[(n, b, region)]

    return get


def device_files(tools, cohorts, tmp_path, n, b, k, region, inflate="host", level="fast", rows_per_call=0, plain=False):
    fasta, bams, ids = cohorts(n)
    prefix = str(tmp_path / "d")
    extra = ["-B", str(b), "--rows", "device", "--batches-per-pass", str(k), "--inflate", inflate, "--deflate-level", level]
    extra += ["--rows-per-call", str(rows_per_call)] if rows_per_call else []
    p = pileup(tools[0], fasta, bams, region, prefix, extra + (["--output-plain"] if plain else []))
    bn = (n + b - 1) // b
    passes = (bn + k - 1) // k if k else 1
    assert "%d batchfiles of %d samples, %d passes, " % (bn, b, passes) in p.stderr, p.stderr
    assert ("BAM members inflated on the device" in p.stderr) == (inflate == "device")
    names = batch_names(prefix, n, b, ".bf" if plain else ".bf.gz")
    return names, [open(f, "rb").read() for f in names]


@pytest.mark.parametrize("inflate,level,rows_per_call", VARIANTS)
@pytest.mark.parametrize("k", PER_PASS)
@pytest.mark.parametrize("n,b", BATCHES)
def test_device_batches_inflate_to_the_host_batches(tools, cohorts, host_files, tmp_path, n, b, k, inflate, level, rows_per_call):
    want = host_files(n, b, REGION)
    names, got = device_files(tools, cohorts, tmp_path, n, b, k, REGION, inflate, level, rows_per_call)
    assert len(got) == len(want) == (n + b - 1) // b
    for name, g, w in zip(names, got, want):
        assert gzip.decompress(g) == w, name
        assert g[-28:-26] == b"\x1f\x8b" and w.count(b"\n") > 201  # the end-of-file member; header and rows


@pytest.mark.parametrize("k", PER_PASS)
@pytest.mark.parametrize("n,b", BATCHES)
def test_device_batches_across_the_step_edge(tools, cohorts, host_files, tmp_path, n, b, k):
    """two windows whatever their size: 499900-500000 and 500001-500100; plain files are the inflated host files themselves"""
    want = host_files(n, b, EDGE)
    names, got = device_files(tools, cohorts, tmp_path, n, b, k, EDGE, "device" if k == 3 else "host", plain=True)
    assert got == want and all(w.count(b"\n") == 3 + 201 for w in want)
    if k != 1:  # and a window size of its own
        fasta, bams, ids = cohorts(n)
        prefix = str(tmp_path / "w")
        pileup(tools[0], fasta, bams, EDGE, prefix, ["-B", str(b), "--rows", "device", "--batches-per-pass", str(k), "--window", "64", "--output-plain"])
        assert [open(f, "rb").read() for f in batch_names(prefix, n, b, ".bf")] == want


@pytest.mark.parametrize("n,b", BATCHES)
def test_bv_call_reads_the_batches_as_it_reads_the_whole_cohort(tools, cohorts, tmp_path, n, b):
    # (the rows behind 1800 hold the indels of the corpus's empty reads: their quality, 255, is written as the byte 0x20, a row
    # that no batchfile reader takes, whichever route wrote it)
    fasta, bams, ids = cohorts(n)
    region = "chr1:900-1800"
    whole = str(tmp_path / "whole.bf.gz")
    pileup(tools[0], fasta, bams, region, whole)
    prefix = str(tmp_path / "b")
    pileup(tools[0], fasta, bams, region, prefix, ["-B", str(b), "--rows", "device", "--batches-per-pass", "3"])
    outs = []
    for tag, files in (("whole", [whole]), ("batches", batch_names(prefix, n, b))):
        v, c = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".cvg"))
        p = subprocess.run([tools[1], "--batchfiles", ",".join(files), "--output-vcf", v, "--output-cvg", c], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append((open(v, "rb").read(), open(c, "rb").read()))
    assert outs[0] == outs[1] and outs[0][1].count(b"\n") > 600
