"""GPU tests of `bv_call --deflate device` (the whole blocks of the *.vcf.gz / *.cvg.gz outputs compressed by
bv_engine_bgzf_deflate) against `bv_call` as it is by default (one zlib deflate() a block on the emitter thread): the files
inflate to the same bytes in the same blocks, every line lies at the same place in its block, and both indexes point at
their lines."""
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
from test_host_formats import cxx, make_batchfiles  # noqa: E402

ARGS = ["--contig", "chr17:81195210", "--reference", "hg19.fa"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cxx(os.path.join(ROOT, "basevar_amd", "host", "bv_call.cpp"), str(tmp_path_factory.mktemp("bin") / "bv_call"), ["-lz"])


def call(exe, files, tag, tmp_path, extra=(), gz=True, expect=0):
    sfx = ".gz" if gz else ""
    v, c, t = str(tmp_path / (tag + ".vcf" + sfx)), str(tmp_path / (tag + ".cvg" + sfx)), str(tmp_path / (tag + ".json"))
    p = subprocess.run([exe, "--batchfiles", ",".join(files), "--output-vcf", v, "--output-cvg", c, "--timing", t] + ARGS + list(extra),
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == expect, (p.returncode, p.stderr[-2000:])
    return v, c, (json.load(open(t)) if expect == 0 else None), p


def whole_blocks(path):
    import bam_py
    return sum(1 for _, _, payload in bam_py.bgzf_blocks(path) if len(payload) == dc.MAX_BLOCK)


def check_pair(want, got, header_blocks=None):
    for which in (0, 1):
        dc.assert_same_text_and_places(want[which], got[which])
    t = got[2]
    assert t["deflate"] == "device" and t["deflate_s"] > 0 and want[2].get("deflate") is None
    # every whole block behind the headers' went through the device
    total = whole_blocks(got[0]) + whole_blocks(got[1])
    assert 0 < t["members_deflated"] <= total
    if header_blocks is not None:
        assert t["members_deflated"] == total - header_blocks
    assert "[NOTE]" not in got[3].stderr


def test_device_deflate_writes_the_default_paths_text_in_the_same_blocks(exe, tmp_path):
    paths, ids, _ = make_batchfiles(tmp_path, n_sites=600, n_samples=400, n_files=4)
    want = call(exe, paths, "host", tmp_path)
    assert os.path.getsize(want[0]) > 20000 and whole_blocks(want[0]) > 3
    # (the headers are shorter than a block here: no whole block is theirs)
    assert len(gzip.open(want[0], "rb").read().split(b"\n#CHROM")[0]) < dc.MAX_BLOCK
    for tag, more in (("t1", ["--thread", "1"]), ("t4", ["--thread", "4"]), ("b7", ["--thread", "4", "--batch-sites", "7"])):
        got = call(exe, paths, tag, tmp_path, more + ["--deflate", "device"])
        check_pair(want, got, header_blocks=0)
        # the device wrote other bytes than zlib: the comparison above is not one of a file with itself
        assert open(got[0], "rb").read() != open(want[0], "rb").read()


def test_ten_thousand_samples_from_the_generator(exe, tmp_path):
    gen = str(tmp_path / "gen_batchfiles")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gen_batchfiles.cpp"), "-lz", "-o", gen])
    d = tmp_path / "bf"
    d.mkdir()
    subprocess.check_call([gen, str(d), "10000", "200", "300"])
    files = sorted(str(d / f) for f in os.listdir(d) if f.endswith(".gz"))
    assert len(files) == 50
    want = call(exe, files, "host", tmp_path, ["--thread", "4"])
    for tag, more in (("t1", ["--thread", "1"]), ("t4", ["--thread", "4"]), ("b16", ["--thread", "4", "--batch-sites", "16"])):
        got = call(exe, files, tag, tmp_path, more + ["--deflate", "device"])
        check_pair(want, got)
    assert whole_blocks(want[0]) > 20
    # with the device inflate in front as well
    got = call(exe, files, "both", tmp_path, ["--thread", "4", "--deflate", "device", "--inflate", "device"])
    check_pair(want, got)


def test_outputs_and_values_the_flag_does_not_apply_to(exe, tmp_path):
    paths, _, _ = make_batchfiles(tmp_path, n_sites=200, n_samples=60)
    want = call(exe, paths, "host", tmp_path, gz=False)
    got = call(exe, paths, "dev", tmp_path, ["--deflate", "device"], gz=False)
    for which in (0, 1):
        assert open(got[which], "rb").read() == open(want[which], "rb").read()
    assert got[3].stderr.count("[NOTE] --deflate device") == 1 and got[2].get("deflate") is None and "members_deflated" not in got[2]
    same = call(exe, paths, "hostflag", tmp_path, ["--deflate", "host"], gz=False)
    assert open(same[0], "rb").read() == open(want[0], "rb").read() and "[NOTE]" not in same[3].stderr and same[2].get("deflate") is None
    bad = subprocess.run([exe, "--batchfiles", ",".join(paths), "--output-vcf", str(tmp_path / "x.vcf.gz"), "--output-cvg", str(tmp_path / "x.cvg.gz"),
                          "--deflate", "gpu"] + ARGS, capture_output=True, text=True)
    assert bad.returncode == 1 and "--deflate wants device or host" in bad.stderr
