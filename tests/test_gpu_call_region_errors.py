"""GPU test of bv_call's region errors on BAM input.  A region that does not lie inside its contig is found by the producer, while
the engine workers and the emitter run (the tool makes its engines before it reads a region: that is all this needs a GPU for):
it ends the run the orderly way -- queues closed, threads joined, outputs closed -- with its message and exit status 1, so the
`*.gz` outputs that were opened are complete BGZF files.  A region that is not CHR:BEG-END is refused before any thread exists."""
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
from test_gpu_vcf_emit_call import exe  # noqa: E402,F401

BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


@pytest.fixture(scope="module")
def bam_args(tmp_path_factory):
    fasta, bams, _ = cohort(tmp_path_factory.mktemp("cohort"), 3)
    return sum((["-I", b] for b in bams), []) + ["-R", fasta, "-q", str(pr.MAPQ_THD), "--thread", "2"]


def run(exe, args, regions, tmp_path, tag, extra=()):  # noqa: F811
    v, c = str(tmp_path / (tag + ".vcf.gz")), str(tmp_path / (tag + ".cvg.gz"))
    p = subprocess.run([exe] + args + ["-r", regions, "--output-vcf", v, "--output-cvg", c] + list(extra), capture_output=True, text=True, timeout=300)
    return p, v, c


@pytest.mark.parametrize("pileup", ["host", "device"])
def test_region_outside_its_contig_ends_the_run_in_order(exe, bam_args, tmp_path, pileup):  # noqa: F811
    name, length = pr.REFS[1]
    p, v, c = run(exe, bam_args, "%s:1-%d" % (name, length + 1), tmp_path, pileup, ["--pileup", pileup])
    assert p.returncode == 1, (p.returncode, p.stderr[-2000:])
    assert p.stderr.strip().splitlines()[-1] == "[ERROR] region outside " + name and "[INFO]" not in p.stdout
    for path, first in ((v, b"##fileformat=VCF"), (c, b"##fileformat=CVG")):
        raw = open(path, "rb").read()
        assert raw.endswith(BGZF_EOF) and len(raw) > len(BGZF_EOF)
        assert gzip.decompress(raw).startswith(first)  # (every member inflates, the end-of-file member included)


def test_region_that_is_not_chr_beg_end_is_refused(exe, bam_args, tmp_path):  # noqa: F811
    p, v, c = run(exe, bam_args, "%s:1-50,nonsense" % pr.REFS[1][0], tmp_path, "syntax")
    assert p.returncode == 1, (p.returncode, p.stderr[-2000:])
    assert p.stderr.strip() == "--regions wants CHR:BEG-END[,CHR:BEG-END...]"
