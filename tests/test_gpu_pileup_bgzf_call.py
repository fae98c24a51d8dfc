"""GPU tests of the tools' `--inflate device` on BAM input (host/raw_members.hpp + bv_engine_pileup_bgzf): `bv_call --pileup device
--inflate device` writes the VCF and the CVG of `--pileup device` alone, byte for byte; `bv_pileup --rows device --inflate device`
writes a batchfile that inflates to the default route's bytes; `--timing` counts the members; where the route does not apply a
note is printed and nothing changes."""
import gzip
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bai_py  # noqa: E402
import pileup_ref as pr  # noqa: E402
from test_gpu_pileup_call import call, cohort  # noqa: E402
from test_gpu_pileup_text_call import pileup, tools  # noqa: E402,F401
from test_gpu_vcf_emit_call import exe  # noqa: E402,F401

REGIONS = "chr1:900-2300,chr1:499900-500100"


@pytest.fixture(scope="module", params=[3, 130])
def cohort_n(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("pbgzf_cohort_%d" % request.param)
    return (request.param,) + cohort(d, request.param)


def test_bv_call_inflate_device_writes_pileup_devices_vcf_and_cvg(exe, cohort_n, tmp_path):  # noqa: F811
    """two regions (the second across the 500 kb step edge), with and without pop-groups"""
    n, fasta, bams, ids = cohort_n
    groups = tmp_path / "groups.txt"
    groups.write_text("".join("%s\tpop%d\n" % (s, i % 2) for i, s in enumerate(ids)))
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", REGIONS, "-q", str(pr.MAPQ_THD), "--thread", "4"]
    for tag, more in (("plain", ["--batch-sites", "300"]), ("grp", ["--pop-group", str(groups)])):
        want = call(exe, args + more, tag + "_dev", tmp_path, ["--pileup", "device"])
        got = call(exe, args + more, tag + "_inf", tmp_path, ["--pileup", "device", "--inflate", "device"])
        assert got[0] == want[0] and got[1] == want[1]
        assert want[0].count(b"\n") > 30 and want[1].count(b"\n") > 1200
        t = got[2]
        assert t["pileup"] == "device" and t["bam_inflate"] == "device" and t["members_inflated"] > 0 and t["members_bytes"] > 26 * t["members_inflated"]
        assert t["sites"] == want[2]["sites"] > 1200 and t["vcf_records"] == want[2]["vcf_records"] and "bam_inflate" not in want[2]
        assert "[NOTE]" not in got[3].stderr


def test_bv_call_on_indexed_files(exe, tmp_path):  # noqa: F811
    """the same through BAI chunks: fewer members cross than from the files' scan"""
    fasta, bams, ids = cohort(tmp_path, 9)
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", REGIONS, "-q", str(pr.MAPQ_THD), "--thread", "2"]
    scan = call(exe, args, "scan", tmp_path, ["--pileup", "device", "--inflate", "device"])
    for b in bams:
        bai_py.write_bai(b)
    want = call(exe, args, "dev", tmp_path, ["--pileup", "device"])
    got = call(exe, args, "inf", tmp_path, ["--pileup", "device", "--inflate", "device"])
    assert got[0] == want[0] == scan[0] and got[1] == want[1] == scan[1] and want[1].count(b"\n") > 1200
    assert 0 < got[2]["members_inflated"] < scan[2]["members_inflated"]


def test_bv_call_inflate_device_without_pileup_device_keeps_its_note_and_path(exe, tmp_path):  # noqa: F811
    fasta, bams, ids = cohort(tmp_path, 3)
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", "chr1:900-1300", "-q", str(pr.MAPQ_THD)]
    want = call(exe, args, "host", tmp_path)
    got = call(exe, args, "inf", tmp_path, ["--inflate", "device"])
    assert got[0] == want[0] and got[1] == want[1] and "bam_inflate" not in got[2]
    assert "[NOTE] --inflate device applies to BGZF batchfiles, not to BAM input" in got[3].stderr


def test_bv_call_takes_the_host_read_for_members_of_another_packing(exe, tmp_path):  # noqa: F811
    """a file whose first member has a longer extra field: a note, and the records come through the host reader"""
    fasta, bams, ids = cohort(tmp_path, 3)
    raw = open(bams[1], "rb").read()
    total = int.from_bytes(raw[16:18], "little") + 1
    wide = raw[:10] + (10).to_bytes(2, "little") + raw[12:16] + (total + 4 - 1).to_bytes(2, "little") + b"XY\0\0" + raw[18:]
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", "chr1:900-1300", "-q", str(pr.MAPQ_THD)]
    want = call(exe, args, "dev", tmp_path, ["--pileup", "device"])
    with open(bams[1], "wb") as f:
        f.write(wide)
    got = call(exe, args, "inf", tmp_path, ["--pileup", "device", "--inflate", "device"])
    assert got[0] == want[0] and got[1] == want[1] and "bam_inflate" not in got[2] and got[2]["pileup"] == "device"
    assert "[NOTE] --inflate device: the BGZF members of " + bams[1] in got[3].stderr


def test_bv_pileup_inflate_device_writes_the_default_routes_batchfile(tools, cohort_n, tmp_path):  # noqa: F811
    n, fasta, bams, ids = cohort_n
    for region in ("chr1:900-2300", "chr1:499900-500100", "chr1:300000-300070"):
        want = pileup(tools[0], fasta, bams, region, tmp_path / "host.bf")
        got_gz = pileup(tools[0], fasta, bams, region, tmp_path / "inf.bf.gz", ["--rows", "device", "--inflate", "device", "--window", "512"])
        assert gzip.decompress(got_gz) == want and want.count(b"\n") > 71
    assert pileup(tools[0], fasta, bams, "chr1:900-2300", tmp_path / "inf.bf", ["--rows", "device", "--inflate", "device"]) == pileup(tools[0], fasta, bams, "chr1:900-2300", tmp_path / "h.bf")


def test_bv_pileup_says_what_it_inflated_and_where_it_does_not_apply(tools, tmp_path):  # noqa: F811
    import subprocess
    fasta, bams, ids = cohort(tmp_path, 3)
    base = [tools[0], "-R", fasta, "--regions", "chr1:900-1300", "-q", str(pr.MAPQ_THD)] + sum((["-I", b] for b in bams), [])
    p = subprocess.run(base + ["-o", str(tmp_path / "a.bf"), "--rows", "device", "--inflate", "device"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "BAM members inflated on the device: " in p.stderr and "inflated on the device: 0 " not in p.stderr and "[NOTE]" not in p.stderr
    q = subprocess.run(base + ["-o", str(tmp_path / "b.bf"), "--inflate", "device"], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0 and "[NOTE] --inflate device takes effect with --rows device" in q.stderr and "inflated on the device" not in q.stderr
    assert open(str(tmp_path / "a.bf"), "rb").read() == open(str(tmp_path / "b.bf"), "rb").read()
    r = subprocess.run(base + ["-o", str(tmp_path / "c.bf"), "--inflate", "sideways"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "--inflate wants host or device" in r.stderr
