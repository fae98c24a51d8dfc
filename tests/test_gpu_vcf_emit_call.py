"""GPU tests of `bv_call --emit device` (the VCF lines' sample columns written by the worker's engine from the rows its text
submit left on the device, a *.vcf.gz deflated there too: bv_engine_vcf_format / _deflate) against the same run without the
flag: the VCF inflates to the same bytes, the CVG file is the same file, and the index points at every VCF line."""
import gzip
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_corpus as dc  # noqa: E402
from test_gpu_bgzf_call import as_bgzf  # noqa: E402
from test_host_formats import LIB, cxx, make_batchfiles  # noqa: E402

ARGS = ["--contig", "chr17:81195210", "--reference", "hg19.fa"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """bv_call from this tree's source, against the built library (built first where it is missing)"""
    src, out = os.path.join(ROOT, "basevar_amd", "host", "bv_call.cpp"), str(tmp_path_factory.mktemp("bin") / "bv_call")
    if not os.path.exists(os.path.join(LIB, "libbasevar_amd.so")):
        return cxx(src, out, ["-lz"])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-L", LIB, "-lbasevar_amd", "-Wl,-rpath," + LIB,
                           "-pthread", "-o", out, "-lz"])
    return out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """300 positions x 400 samples in four BGZF batchfiles, and a pop-group file of two groups"""
    d = tmp_path_factory.mktemp("bf")
    paths, ids, _ = make_batchfiles(d, n_sites=300, n_samples=400, n_files=4)
    groups = d / "groups.txt"
    groups.write_text("".join("%s\tpop%d\n" % (s, i % 2) for i, s in enumerate(ids)))
    return as_bgzf(paths), str(groups)


def call(exe, inputs_args, tag, tmp_path, extra=(), gz=True):
    sfx = ".gz" if gz else ""
    v, c, t = str(tmp_path / (tag + ".vcf" + sfx)), str(tmp_path / (tag + ".cvg" + sfx)), str(tmp_path / (tag + ".json"))
    p = subprocess.run([exe] + inputs_args + ["--output-vcf", v, "--output-cvg", c, "--timing", t] + list(extra), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return v, c, json.load(open(t)), p


def check_gz_pair(want, got):
    """the run with --emit device against the same run without it"""
    text = gzip.open(got[0], "rb").read()
    assert text == gzip.open(want[0], "rb").read()
    assert open(got[1], "rb").read() == open(want[1], "rb").read()          # the CVG file: byte-identical
    assert open(got[1] + ".tbi", "rb").read() == open(want[1] + ".tbi", "rb").read()
    # every VCF data line through the index, by the independent reader; the same lines as the other run's
    lines = dc.indexed_lines(got[0])
    assert [l for _, _, l in lines] == [l for _, _, l in dc.indexed_lines(want[0])]
    n_records = sum(1 for _, _, l in lines if not l.startswith(b"#"))
    t = got[2]
    assert t["emit"] == "device" and t["vcf_lines_device"] == t["vcf_records"] == n_records > 20
    assert want[2].get("emit") is None and want[2]["vcf_records"] == n_records
    assert "[NOTE]" not in got[3].stderr
    return text


@pytest.mark.parametrize("inflate", ["host", "device"])
@pytest.mark.parametrize("level", ["fast", "small"])
def test_emit_device_writes_the_same_vcf_and_the_same_cvg_file(exe, inputs, tmp_path, inflate, level):
    files, groups = inputs
    base = ["--batchfiles", ",".join(files)] + ARGS
    flags = ["--inflate", inflate, "--deflate", "device", "--deflate-level", level, "--thread", "4"]
    for tag, more in (("b7", ["--batch-sites", "7"]), ("grp", ["--pop-group", groups, "--batch-sites", "64"])):
        want = call(exe, base, tag + "_want", tmp_path, flags + more)
        got = call(exe, base, tag + "_got", tmp_path, flags + more + ["--emit", "device"])
        text = check_gz_pair(want, got)
        assert (b";pop0_AF=" in text and b";pop1_AF=" in text) == ("--pop-group" in more)
        # the members are cut from each batch's first byte: other cuts than the host writer's, at least one short member a batch
        assert open(got[0], "rb").read() != open(want[0], "rb").read()


def test_emit_device_without_device_deflate_and_into_plain_files(exe, inputs, tmp_path):
    """--emit device alone, against bv_call as it is by default: the CVG file stays with zlib; plain *.vcf / *.cvg outputs are
    the default run's bytes"""
    files, groups = inputs
    base = ["--batchfiles", ",".join(files)] + ARGS
    want = call(exe, base, "want", tmp_path, ["--batch-sites", "50"])
    got = call(exe, base, "got", tmp_path, ["--batch-sites", "50", "--emit", "device"])
    check_gz_pair(want, got)
    want = call(exe, base, "pwant", tmp_path, ["--batch-sites", "50"], gz=False)
    for inflate in ("host", "device"):
        got = call(exe, base, "pgot_" + inflate, tmp_path, ["--batch-sites", "50", "--emit", "device", "--inflate", inflate], gz=False)
        for which in (0, 1):
            assert open(got[which], "rb").read() == open(want[which], "rb").read()
        assert got[2]["emit"] == "device" and got[2]["vcf_lines_device"] == got[2]["vcf_records"] > 20
    bad = subprocess.run([exe] + base + ["--output-vcf", str(tmp_path / "x.vcf"), "--output-cvg", str(tmp_path / "x.cvg"), "--emit", "gpu"],
                         capture_output=True, text=True)
    assert bad.returncode == 1 and "--emit wants device or host" in bad.stderr


def test_bam_input_takes_the_host_path_and_says_so(exe, tmp_path):
    data = os.path.join(ROOT, "tests", "golden", "data")
    bam = os.path.join(data, "range.bam")
    base = ["-I", bam, "-I", bam, "-R", os.path.join(data, "ce.fa.gz"), "--regions", "CHROMOSOME_I:900-1200", "--mapq", "10", "--min-af", "0.05",
            "--batch-sites", "64"]
    want = call(exe, base, "want", tmp_path)
    got = call(exe, base, "got", tmp_path, ["--emit", "device"])
    for which in (0, 1):
        assert open(got[which], "rb").read() == open(want[which], "rb").read()
        assert open(got[which] + ".tbi", "rb").read() == open(want[which] + ".tbi", "rb").read()
    assert got[3].stderr.count("[NOTE] --emit device") == 1 and got[2].get("emit") is None and "vcf_lines_device" not in got[2]
    assert got[2]["vcf_records"] == 5
