"""GPU tests of `bv_call --pileup device` (the samples' raw BAM records piled up, gathered and submitted on an engine of the
producer's own: bv_engine_pileup / _rows / _submit) against the same run without the flag: the VCF and the CVG are the same
bytes; `--timing` says so; batchfile input prints a note and is unchanged."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_py  # noqa: E402
import pileup_ref as pr  # noqa: E402
from test_gpu_vcf_emit_call import exe  # noqa: E402,F401
from test_host_formats import make_batchfiles  # noqa: E402


def cohort(directory, n):
    """n BAM files of the pileup corpus (sample 0 the special one), each with a sample name of its own, and their FASTA"""
    fa = pr.reference()
    fasta = os.path.join(str(directory), "ref.fa")
    pr.write_fasta(fasta, fa)
    paths, ids = [], []
    for s in range(n):
        rng = np.random.default_rng(400 + s)
        recs = pr.special_sample(rng) if s == 0 else ([] if s % 7 == 3 else pr.random_sample(rng))
        header = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in pr.REFS) + "@RG\tID:x\tSM:smp%03d\n" % s
        path = os.path.join(str(directory), "s%03d.bam" % s)
        bam_py.write_bam(path, pr.REFS, recs, header_text=header, block_payload=700 if s < 3 else 60000)
        paths.append(path)
        ids.append("smp%03d" % s)
    return fasta, paths, ids


def call(exe, args, tag, tmp_path, extra=()):  # noqa: F811
    v, c, t = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".cvg")), str(tmp_path / (tag + ".json"))
    p = subprocess.run([exe] + args + ["--output-vcf", v, "--output-cvg", c, "--timing", t] + list(extra), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return open(v, "rb").read(), open(c, "rb").read(), json.load(open(t)), p


@pytest.mark.parametrize("n", [3, 130])
def test_pileup_device_writes_the_default_runs_vcf_and_cvg(exe, tmp_path, n):  # noqa: F811
    """two regions (the second across the 500 kb step edge), batches smaller than a window's covered rows, with and without pop-groups"""
    fasta, bams, ids = cohort(tmp_path, n)
    groups = tmp_path / "groups.txt"
    groups.write_text("".join("%s\tpop%d\n" % (s, i % 2) for i, s in enumerate(ids)))
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", "chr1:900-2300,chr1:499900-500100", "-q", str(pr.MAPQ_THD), "--thread", "4"]
    for tag, more in (("plain", ["--batch-sites", "300"]), ("grp", ["--pop-group", str(groups)])):
        want = call(exe, args + more, tag + "_host", tmp_path)
        got = call(exe, args + more, tag + "_dev", tmp_path, ["--pileup", "device"])
        assert got[0] == want[0] and got[1] == want[1]
        assert want[0].count(b"\n") > 30 and want[1].count(b"\n") > 1200  # header lines, records and covered positions are there
        t = got[2]
        assert t["pileup"] == "device" and t["reads_bytes"] > 1000 * min(n, 100) and t["pileup_s"] > 0 and t["sites"] == want[2]["sites"] > 1200
        assert t["vcf_records"] == want[2]["vcf_records"] and "pileup" not in want[2]
        assert "[NOTE]" not in got[3].stderr


def test_pileup_device_on_batchfiles_prints_a_note_and_changes_nothing(exe, tmp_path):  # noqa: F811
    paths, ids, _ = make_batchfiles(tmp_path, n_sites=60, n_samples=40, n_files=2)
    args = ["--batchfiles", ",".join(paths), "--contig", "chr17:81195210", "--reference", "hg19.fa"]
    want = call(exe, args, "host", tmp_path)
    got = call(exe, args, "dev", tmp_path, ["--pileup", "device"])
    assert got[0] == want[0] and got[1] == want[1] and "pileup" not in got[2]
    assert "[NOTE] --pileup device applies to BAM input" in got[3].stderr and "[NOTE]" not in want[3].stderr
