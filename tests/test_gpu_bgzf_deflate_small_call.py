"""GPU tests of `bv_call --deflate device --deflate-level small` (the whole blocks of the *.vcf.gz / *.cvg.gz outputs
compressed by bv_engine_bgzf_deflate_level at BV_DEFLATE_SMALL) against `bv_call` as it is by default: the files inflate to
the same bytes in the same blocks, every line lies at the same place in its block, both indexes point at their lines, and the
.vcf.gz is smaller than the fast level's."""
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


def call(exe, files, tag, tmp_path, extra=(), expect=0):
    v, c, t = str(tmp_path / (tag + ".vcf.gz")), str(tmp_path / (tag + ".cvg.gz")), str(tmp_path / (tag + ".json"))
    p = subprocess.run([exe, "--batchfiles", ",".join(files), "--output-vcf", v, "--output-cvg", c, "--timing", t] + ARGS + list(extra),
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == expect, (p.returncode, p.stderr[-2000:])
    return v, c, (json.load(open(t)) if expect == 0 else None), p


def test_the_small_level_writes_the_default_paths_text_in_the_same_blocks_and_a_smaller_file(exe, tmp_path):
    paths, _, _ = make_batchfiles(tmp_path, n_sites=600, n_samples=400, n_files=4)
    want = call(exe, paths, "host", tmp_path)
    fast = call(exe, paths, "fast", tmp_path, ["--deflate", "device"])
    named = call(exe, paths, "named", tmp_path, ["--deflate", "device", "--deflate-level", "fast"])
    small = call(exe, paths, "small", tmp_path, ["--deflate", "device", "--deflate-level", "small"])
    for which in (0, 1):
        dc.assert_same_text_and_places(want[which], small[which])
        assert open(named[which], "rb").read() == open(fast[which], "rb").read()
    assert os.path.getsize(small[0]) < os.path.getsize(fast[0]) and os.path.getsize(small[1]) <= os.path.getsize(fast[1])
    print("vcf.gz: host %d B, fast %d B, small %d B" % tuple(os.path.getsize(x[0]) for x in (want, fast, small)))
    t = small[2]
    assert t["deflate"] == "device" and t["deflate_level"] == "small" and t["deflate_s"] > 0 and t["members_deflated"] == fast[2]["members_deflated"] > 0
    assert fast[2]["deflate_level"] == "fast" and named[2]["deflate_level"] == "fast" and "deflate_level" not in want[2]


def test_the_level_is_an_error_on_the_host_path_and_for_other_names(exe, tmp_path):
    paths, _, _ = make_batchfiles(tmp_path, n_sites=40, n_samples=20)
    for extra, message in ((["--deflate", "host", "--deflate-level", "small"], "--deflate-level small needs --deflate device"),
                           (["--deflate-level", "small"], "--deflate-level small needs --deflate device"),
                           (["--deflate", "device", "--deflate-level", "best"], "--deflate-level wants fast or small")):
        _, _, _, p = call(exe, paths, "bad", tmp_path, extra, expect=1)
        assert message in p.stderr, p.stderr[-500:]
        assert not os.path.exists(tmp_path / "bad.vcf.gz")
    call(exe, paths, "ok", tmp_path, ["--deflate", "host", "--deflate-level", "fast"])
