"""GPU tests of `bv_call -I ... --pileup device --emit device` (the VCF records and the CVG rows written on the pileup's engine
from the records and the rows where they lie: bv_engine_vcf_format_records, bv_engine_cvg_format), with and without
`--inflate device`, against the default run: the VCF inflates to the same bytes, the CVG is the same file, the index finds
every line, `--timing` says what the device wrote and what the host formatted, and no note is printed."""
import gzip
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
import deflate_corpus as dc  # noqa: E402
import pileup_ref as pr  # noqa: E402
from test_gpu_pileup_call import cohort  # noqa: E402
from test_gpu_vcf_emit_call import exe  # noqa: E402,F401


def call(exe, args, tag, tmp_path, extra=(), gz=False):  # noqa: F811
    sfx = ".gz" if gz else ""
    v, c, t = str(tmp_path / (tag + ".vcf" + sfx)), str(tmp_path / (tag + ".cvg" + sfx)), str(tmp_path / (tag + ".json"))
    p = subprocess.run([exe] + args + ["--output-vcf", v, "--output-cvg", c, "--timing", t] + list(extra), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return v, c, json.load(open(t)), p


def same_outputs(want, got, gz):
    if gz:
        assert gzip.open(got[0], "rb").read() == gzip.open(want[0], "rb").read()
        assert open(got[1], "rb").read() == open(want[1], "rb").read()  # the CVG file: the same bytes, compressed
        assert open(got[1] + ".tbi", "rb").read() == open(want[1] + ".tbi", "rb").read()
        lines = dc.indexed_lines(got[0])  # every VCF line through the index, by the independent reader
        assert [l for _, _, l in lines] == [l for _, _, l in dc.indexed_lines(want[0])]
    else:
        for which in (0, 1):
            assert open(got[which], "rb").read() == open(want[which], "rb").read()


def check_timing(want, got):
    t = got[2]
    assert t["emit"] == "device" and t["pileup"] == "device" and t["vcf_lines_device"] == t["vcf_records"] == want[2]["vcf_records"] > 20
    assert t["sites"] == want[2]["sites"] and t["cvg_lines_device"] + t["lines_host_formatted"] >= t["sites"] > 1200
    assert want[2].get("emit") is None
    assert "[NOTE]" not in got[3].stderr


@pytest.mark.parametrize("n", [3, 130])
def test_emit_device_on_bam_input_writes_the_default_runs_files(exe, tmp_path, n):  # noqa: F811
    fasta, bams, ids = cohort(tmp_path, n)
    groups = tmp_path / "groups.txt"
    groups.write_text("".join("%s\tpop%d\n" % (s, i % 2) for i, s in enumerate(ids)))
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", "chr1:900-2300,chr1:499900-500100", "-q", str(pr.MAPQ_THD), "--thread", "4"]
    for tag, more, gz in (("plain", ["--batch-sites", "300"], False), ("grp", ["--pop-group", str(groups)], True)):
        want = call(exe, args + more, tag + "_host", tmp_path, gz=gz)
        for inflate in ("host", "device"):
            got = call(exe, args + more, tag + "_dev_" + inflate, tmp_path, ["--pileup", "device", "--emit", "device", "--inflate", inflate], gz=gz)
            same_outputs(want, got, gz)
            check_timing(want, got)
            # (the reference's run of five N: a site there can have four ALTs, one more than the device formats)
            assert got[2]["lines_host_formatted"] <= 5 and (n > 3 or got[2]["lines_host_formatted"] == 0)
            assert (got[2].get("bam_inflate") == "device") == (inflate == "device")
    assert b";pop0_AF=" in gzip.open(got[0], "rb").read()
    # with --deflate device the CVG text goes through the device's deflate as the host-formatted text does
    want = call(exe, args, "dd_host", tmp_path, ["--pileup", "device", "--deflate", "device"], gz=True)
    got = call(exe, args, "dd_dev", tmp_path, ["--pileup", "device", "--deflate", "device", "--emit", "device"], gz=True)
    same_outputs(want, got, True)


def test_a_q0_base_is_formatted_by_the_host(exe, tmp_path):  # noqa: F811
    """a read of quality 0 at every base, none of them the reference's, where no other read lies: AF = NaN at its sites (SURVEY
    section 8a; the site of tests/golden/edge16.npz is of this kind)"""
    fasta, bams, ids = cohort(tmp_path, 3)
    fa = pr.reference()
    rng = np.random.default_rng(9)
    seq = "".join("ACGT"[("ACGT".index(c.upper()) + 1) % 4] if c.upper() in "ACGT" else "A" for c in fa[300000:300040])
    recs = [pr.read(rng, 300000, [(pr.M, 40)], seq=seq, qual=[0] * 40)]
    header = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in pr.REFS) + "@RG\tID:x\tSM:q0\n"
    path = os.path.join(str(tmp_path), "q0.bam")
    bam_py.write_bam(path, pr.REFS, recs, header_text=header, block_payload=60000)
    args = sum((["-I", b] for b in bams + [path]), []) + ["-R", fasta, "-r", "chr1:1600-1800,chr1:299990-300060", "-q", str(pr.MAPQ_THD), "--thread", "2"]
    want = call(exe, args, "host", tmp_path)
    got = call(exe, args, "dev", tmp_path, ["--pileup", "device", "--emit", "device"])
    same_outputs(want, got, False)
    assert got[2]["lines_host_formatted"] >= 1 and got[2]["emit"] == "device" and "[NOTE]" not in got[3].stderr


def test_emit_device_with_the_host_pileup_says_so(exe, tmp_path):  # noqa: F811
    fasta, bams, ids = cohort(tmp_path, 3)
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", "chr1:900-1300", "-q", str(pr.MAPQ_THD)]
    want = call(exe, args, "host", tmp_path)
    got = call(exe, args, "dev", tmp_path, ["--emit", "device"])
    same_outputs(want, got, False)
    assert got[3].stderr.count("[NOTE] --emit device on BAM input needs --pileup device") == 1 and got[2].get("emit") is None
