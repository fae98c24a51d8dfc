"""GPU tests of `bv_call --inflate device` (BGZF batchfiles inflated, split into lines and parsed on the device) against
`bv_call` as it is by default (zlib, line split and row packing on the host): the VCF and CVG files are the same bytes."""
import gzip
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzf_corpus as bc  # noqa: E402
from test_host_formats import cxx, make_batchfiles  # noqa: E402

ARGS = ["--contig", "chr17:81195210", "--reference", "hg19.fa"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cxx(os.path.join(ROOT, "basevar_amd", "host", "bv_call.cpp"), str(tmp_path_factory.mktemp("bin") / "bv_call"), ["-lz"])


def as_bgzf(paths, members=(0xff00, 0x1000, 0x300)):
    """the gzip batchfiles rewritten as BGZF files, another member size per file"""
    out = []
    for k, p in enumerate(paths):
        data = gzip.open(p, "rb").read()
        q = p[:-3] + ".bgzf.gz"
        with open(q, "wb") as fh:
            m = members[k % len(members)]
            for at in range(0, len(data), m):
                fh.write(bc.member(data[at:at + m], 6))
            fh.write(bc.member(b""))
        out.append(q)
    return out


def call(exe, files, tag, tmp_path, extra=(), expect=0):
    v, c, t = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".cvg")), str(tmp_path / (tag + ".json"))
    p = subprocess.run([exe, "--batchfiles", ",".join(files), "--output-vcf", v, "--output-cvg", c, "--timing", t] + ARGS + list(extra),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == expect, (p.returncode, p.stderr[-2000:])
    timing = json.load(open(t)) if expect == 0 else None
    return open(v, "rb").read(), open(c, "rb").read(), timing, p


@pytest.mark.parametrize("n_groups", [0, 2, 40])
def test_device_inflate_writes_the_default_paths_bytes(exe, tmp_path, n_groups):
    paths, ids, _ = make_batchfiles(tmp_path, n_sites=400, n_samples=120)
    files = as_bgzf(paths)
    extra = []
    if n_groups:
        g = tmp_path / "groups.txt"
        g.write_text("".join("%s\tpop%02d\n" % (s, i % n_groups) for i, s in enumerate(ids)))
        extra = ["--pop-group", str(g)]
    want = call(exe, files, "host", tmp_path, extra)
    assert want[2].get("inflate") is None and len(want[1]) > 1000 and want[0].count(b"\n") > 20
    for tag, more in (("t1", ["--thread", "1"]), ("t4", ["--thread", "4"]), ("b5", ["--thread", "4", "--batch-sites", "5"])):
        got = call(exe, files, tag, tmp_path, extra + more + ["--inflate", "device"])
        assert got[0] == want[0] and got[1] == want[1], tag
        assert got[2]["inflate"] == "device" and got[2]["members_inflated"] >= got[2]["members_in_files"] > 0
        assert "[NOTE]" not in got[3].stderr


def test_ten_thousand_samples_from_the_generator(exe, tmp_path):
    gen = str(tmp_path / "gen_batchfiles")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gen_batchfiles.cpp"), "-lz", "-o", gen])
    d = tmp_path / "bf"
    d.mkdir()
    subprocess.check_call([gen, str(d), "10000", "200", "600"])
    files = sorted(str(d / f) for f in os.listdir(d) if f.endswith(".gz"))
    assert len(files) == 50
    want = call(exe, files, "host", tmp_path)
    got = call(exe, files, "dev", tmp_path, ["--inflate", "device", "--thread", "4"])
    assert got[0] == want[0] and got[1] == want[1] and len(want[1]) > 10000
    assert got[2]["inflate"] == "device" and got[2]["members_inflated"] > 50


def test_inputs_the_flag_does_not_apply_to(exe, tmp_path):
    """plain-gzip batchfiles, and two engines: one note, the host path, the same bytes"""
    paths, _, _ = make_batchfiles(tmp_path, n_sites=200, n_samples=60)
    want = call(exe, paths, "host", tmp_path)
    got = call(exe, paths, "gz", tmp_path, ["--inflate", "device"])
    assert got[0] == want[0] and got[1] == want[1] and got[3].stderr.count("[NOTE] --inflate device") == 1 and got[2].get("inflate") is None
    files = as_bgzf(paths)
    got = call(exe, files, "g2", tmp_path, ["--inflate", "device", "--gpus", "2", "--devices", "0,0"])
    assert got[0] == want[0] and got[1] == want[1] and got[3].stderr.count("[NOTE] --inflate device") == 1 and got[2].get("inflate") is None
    bad = subprocess.run([exe, "--batchfiles", ",".join(files), "--output-vcf", str(tmp_path / "x.vcf"), "--output-cvg", str(tmp_path / "x.cvg"),
                          "--inflate", "gpu"] + ARGS, capture_output=True, text=True)
    assert bad.returncode == 1 and "--inflate wants device or host" in bad.stderr


def test_a_file_damaged_midway(exe, tmp_path):
    """a member of file 1 whose DEFLATE stream is damaged half-way through the file: the host path's message, exit status 1,
    and every line written is a line of the good run, in order, from the top"""
    # (files of 15 MB of text each: the damage lies beyond the 4 MiB that the header scan's reader takes in ahead, so both paths
    # meet it in their pipeline)
    gen = str(tmp_path / "gen_batchfiles")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gen_batchfiles.cpp"), "-lz", "-o", gen])
    d = tmp_path / "bf"
    d.mkdir()
    subprocess.check_call([gen, str(d), "600", "200", "6000"])
    files = sorted(str(d / f) for f in os.listdir(d) if f.endswith(".gz"))
    assert len(files) == 3 and os.path.getsize(files[1]) > (1 << 20)
    good = call(exe, files, "good", tmp_path, ["--batch-sites", "500", "--inflate", "device"])
    raw = bytearray(open(files[1], "rb").read())
    at, k = 0, 0
    n_members = sum(1 for _ in _members(raw))
    for off, total in _members(raw):
        if k == n_members // 2:
            at = off + 18 + (total - 26) // 2
        k += 1
    raw[at] ^= 0xFF
    raw[at + 1] ^= 0xFF
    open(files[1], "wb").write(bytes(raw))
    host = call(exe, files, "hbad", tmp_path, ["--batch-sites", "500"], expect=1)
    dev = call(exe, files, "dbad", tmp_path, ["--batch-sites", "500", "--inflate", "device"], expect=1)
    msg = [l for l in host[3].stderr.splitlines() if l.startswith("[ERROR]")]
    assert msg and msg[-1] in dev[3].stderr, (host[3].stderr, dev[3].stderr)
    for which in (0, 1):
        assert good[which].startswith(dev[which]) and dev[which].endswith(b"\n")
    assert 0 < len(dev[1]) < len(good[1])


def _members(raw):
    at = 0
    while at < len(raw):
        total = (raw[at + 16] | (raw[at + 17] << 8)) + 1
        yield at, total
        at += total
