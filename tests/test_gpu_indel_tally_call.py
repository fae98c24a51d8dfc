"""GPU tests of `bv_call --emit device` with the CVG rows' indel columns tallied on the engine (bv_engine_indel_tally,
bv_engine_cvg_format_tallied): BAM input piled up on the device, with and without `--inflate device`, on cohorts of 3 and 130
samples, and batchfile input.  In every run VCF and CVG are the default run's bytes, the CVG text has at least 20 rows whose
indel column is not ".", `--timing`'s indel_columns_device counts exactly those of them that the device wrote, and no note is
printed."""
import gzip
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_py  # noqa: E402
import pileup_ref as pr  # noqa: E402
from test_gpu_pileup_call import cohort  # noqa: E402
from test_gpu_record_text_call import call, same_outputs  # noqa: E402
from test_gpu_vcf_emit_call import ARGS, exe, inputs  # noqa: E402,F401


def indel_rows(cvg_path):
    """rows of the CVG text whose indel column (the ninth) is not '.'"""
    data = gzip.open(cvg_path, "rb").read() if cvg_path.endswith(".gz") else open(cvg_path, "rb").read()
    rows = [ln.split(b"\t") for ln in data.splitlines() if ln and not ln.startswith(b"#")]
    assert rows and all(len(r) == 12 for r in rows)
    return sum(1 for r in rows if r[8] != b".")


def check_indel_columns(want, got):
    """`want`: the default run; `got`: the run with --emit device"""
    n = indel_rows(want[1])
    assert n >= 20
    t = got[2]
    assert t["emit"] == "device" and want[2].get("emit") is None and "indel_columns_device" not in want[2]
    # the count minus the host-formatted rows among them: the device wrote, and tallied, every other one
    assert t["indel_columns_device"] == n - t["indel_columns_host"] and t["indel_columns_host"] <= t["lines_host_formatted"] <= 5
    assert 20 <= t["indel_columns_device"] <= t["cvg_lines_device"]
    assert "[NOTE]" not in got[3].stderr


def indel_samples(directory, n_files=2):
    """BAM files of reads that begin with an insertion or a deletion, 40 anchors inside chr1:1700-2290: the same read in every
    file at the even anchors (counts of n_files), reads of the file's own at the odd ones"""
    fa = pr.reference()
    paths = []
    for f in range(n_files):
        shared, own = np.random.default_rng(77), np.random.default_rng(78 + f)
        recs = []
        for k in range(40):
            rng = own if k % 2 else shared
            cigar = [(pr.I, 1 + k % 5), (pr.M, 12)] if k % 3 else [(pr.D, 1 + k % 4), (pr.M, 12)]
            recs.append(pr.read(rng, 1700 + 14 * k, cigar))
        header = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in pr.REFS) + "@RG\tID:x\tSM:indel%d\n" % f
        path = os.path.join(str(directory), "indel%d.bam" % f)
        bam_py.write_bam(path, pr.REFS, recs, header_text=header, block_payload=700)
        paths.append(path)
    assert len(fa) >= 2300
    return paths


@pytest.mark.parametrize("n", [3, 130])
def test_bam_input_tallies_the_indel_columns_on_the_device(exe, tmp_path, n):  # noqa: F811
    fasta, bams, ids = cohort(tmp_path, n)
    bams = bams + indel_samples(tmp_path)
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", "chr1:900-2300,chr1:499900-500100", "-q", str(pr.MAPQ_THD), "--thread", "4", "--batch-sites", "300"]
    want = call(exe, args, "host", tmp_path)
    for inflate in ("host", "device"):
        got = call(exe, args, "dev_" + inflate, tmp_path, ["--pileup", "device", "--emit", "device", "--inflate", inflate])
        same_outputs(want, got, False)
        check_indel_columns(want, got)
        assert got[2]["pileup"] == "device" and (got[2].get("bam_inflate") == "device") == (inflate == "device")


def test_batchfile_input_tallies_the_indel_columns_on_the_device(exe, inputs, tmp_path):  # noqa: F811
    files, groups = inputs
    base = ["--batchfiles", ",".join(files)] + ARGS + ["--thread", "4"]
    for tag, more, gz in (("b50", ["--batch-sites", "50"], False), ("grp", ["--pop-group", groups, "--batch-sites", "64"], True)):
        want = call(exe, base + more, tag + "_want", tmp_path, gz=gz)
        got = call(exe, base + more, tag + "_got", tmp_path, ["--emit", "device"], gz=gz)
        same_outputs(want, got, gz)
        check_indel_columns(want, got)
        assert got[2]["indel_columns_host"] == 0
