"""GPU tests of `bv_call --batchfiles ... --files-per-pass K` (the batchfiles read file-major, K at a time, a window of
--batch-sites positions a time, every window parsed as one job: include/basevar_amd_text_job.h, host/file_major.hpp): VCF and
CVG are the bytes of the run without the flag -- *.gz outputs after inflation, their .tbi finding every line -- for every K and
window, under --indel-tokens, --emit, --deflate device at both levels and --pop-group, across the step edge, with a host-read
position and with a host reader that throws; --timing counts never more than K open batchfiles; and a cohort with more
batchfiles than the process may hold descriptors is called with the flag and cannot be opened without it."""
import gzip
import json
import os
import resource
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_corpus as dc  # noqa: E402
from test_gpu_pileup_batches_call import BV_PILEUP, EDGE, REGION, pileup  # noqa: E402
from test_gpu_pileup_call import cohort  # noqa: E402
from test_gpu_text_tokens_call import damaged, stopping  # noqa: E402,F401
from test_gpu_vcf_emit_call import ARGS, exe  # noqa: E402,F401
from test_pileup_batches_cpu import batch_names  # noqa: E402

BATCHES = [(3, 1), (130, 7), (130, 64), (130, 200)]  # (cohort, B): 3, 19, 3 and 1 batchfiles


@pytest.fixture(scope="module")
def cohorts(tmp_path_factory):
    made = {}

    def get(n):
        if n not in made:
            made[n] = cohort(tmp_path_factory.mktemp("job_cohort_%d" % n), n)
        return made[n]

    return get


@pytest.fixture(scope="module")
def batchfiles(cohorts, tmp_path_factory):
    """the batchfiles of `bv_pileup --rows host -B b` over a cohort and a region, written once, and the cohort's pop-group file"""
    import __graft_entry__ as g
    if not os.path.exists(BV_PILEUP):
        g.build()
    done = {}

    def get(n, b, region=REGION):
        if (n, b, region) not in done:
            fasta, bams, ids = cohorts(n)
            d = tmp_path_factory.mktemp("job_batches")
            prefix = str(d / "c")
            pileup(BV_PILEUP, fasta, bams, region, prefix, ["-B", str(b), "--rows", "host"])
            groups = d / "groups.txt"
            groups.write_text("".join("%s\tpop%d\n" % (s, i % 2) for i, s in enumerate(ids)))
            done[(n, b, region)] = (batch_names(prefix, n, b), str(groups))
        return done[(n, b, region)]

    return get


def call(exe, files, tag, tmp_path, extra=(), gz=False, ok=True, limit=None):  # noqa: F811
    sfx = ".gz" if gz else ""
    v, c, t = str(tmp_path / (tag + ".vcf" + sfx)), str(tmp_path / (tag + ".cvg" + sfx)), str(tmp_path / (tag + ".json"))
    pre = (lambda: resource.setrlimit(resource.RLIMIT_NOFILE, (limit, resource.getrlimit(resource.RLIMIT_NOFILE)[1]))) if limit else None
    p = subprocess.run([exe, "--batchfiles", ",".join(files)] + ARGS + ["--thread", "4", "--output-vcf", v, "--output-cvg", c, "--timing", t] + list(extra),
                       capture_output=True, text=True, timeout=600, preexec_fn=pre)
    if ok:
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return v, c, json.load(open(t)) if p.returncode == 0 else None, p


def same_outputs(want, got, gz):
    for which in (0, 1):
        if gz:  # after inflation; and the index finds every line
            assert gzip.open(got[which], "rb").read() == gzip.open(want[which], "rb").read()
            assert [l for _, _, l in dc.indexed_lines(got[which])] == [l for _, _, l in dc.indexed_lines(want[which])]
        else:
            assert open(got[which], "rb").read() == open(want[which], "rb").read()


def check_counters(got, K, F, bs=None):
    t = got[2]
    assert t["files_per_pass"] == K and 1 <= t["max_open_batchfiles"] <= min(K, F)
    groups = (F + K - 1) // K
    assert t["passes"] >= groups * ((201 + bs - 1) // bs if bs else 1)  # (windows x groups)
    if bs:
        assert t["batch_sites"] == bs


@pytest.mark.parametrize("k", ["1", "4", "F", "F+5"])
@pytest.mark.parametrize("n,b", BATCHES)
def test_every_k_and_window_writes_the_default_runs_files(exe, batchfiles, tmp_path, n, b, k):  # noqa: F811
    files, groups = batchfiles(n, b)
    F = len(files)
    K = {"1": 1, "4": 4, "F": F, "F+5": F + 5}[k]
    for bs in (1, 64, None):
        more = ["--batch-sites", str(bs)] if bs else []
        want = call(exe, files, "want%s" % bs, tmp_path, more)
        got = call(exe, files, "got%s" % bs, tmp_path, more + ["--files-per-pass", str(K)])
        same_outputs(want, got, False)
        assert want[2]["sites"] == got[2]["sites"] > 100 and "files_per_pass" not in want[2]
        check_counters(got, K, F, bs)
        assert "[NOTE]" not in got[3].stderr


@pytest.mark.parametrize("flags,gz", [
    (["--indel-tokens", "device"], False), (["--emit", "device"], False), (["--indel-tokens", "device", "--emit", "device"], False),
    (["--deflate", "device"], True), (["--deflate", "device", "--deflate-level", "small", "--emit", "device"], True),
    (["--pop-group", "GROUPS"], False), (["--pop-group", "GROUPS", "--emit", "device", "--indel-tokens", "device", "--deflate", "device"], True)],
    ids=["tokens", "emit", "tokens_emit", "deflate_fast", "deflate_small_emit", "groups", "groups_all"])
def test_the_flags_that_work_unchanged(exe, batchfiles, tmp_path, flags, gz):  # noqa: F811
    files, groups = batchfiles(130, 7)
    flags = [groups if f == "GROUPS" else f for f in flags]
    want = call(exe, files, "want", tmp_path, flags + ["--batch-sites", "64"], gz=gz)
    got = call(exe, files, "got", tmp_path, flags + ["--batch-sites", "64", "--files-per-pass", "4"], gz=gz)
    same_outputs(want, got, gz)
    check_counters(got, 4, len(files), 64)
    for key in ("indel_tokens_device", "vcf_lines_device", "cvg_lines_device", "vcf_records", "sites"):
        assert want[2].get(key) == got[2].get(key), key
    assert "[NOTE]" not in got[3].stderr


def test_the_step_edge(exe, batchfiles, tmp_path):  # noqa: F811
    files, groups = batchfiles(130, 64, EDGE)
    want = call(exe, files, "want", tmp_path, ["--batch-sites", "64"])
    got = call(exe, files, "got", tmp_path, ["--batch-sites", "64", "--files-per-pass", "2"])
    same_outputs(want, got, False)
    check_counters(got, 2, len(files))


@pytest.mark.parametrize("emit", ["host", "device"])
@pytest.mark.parametrize("tokens", ["host", "device"])
def test_a_host_read_position(exe, damaged, tmp_path, tokens, emit):  # noqa: F811
    files, at = damaged
    more = ["--batch-sites", "40", "--indel-tokens", tokens, "--emit", emit]
    want = call(exe, files, "want", tmp_path, more)
    for K in (1, 2):
        got = call(exe, files, "got%d" % K, tmp_path, more + ["--files-per-pass", str(K)])
        same_outputs(want, got, False)
        assert got[2].get("indel_tokens_device") == want[2].get("indel_tokens_device")


@pytest.mark.parametrize("tokens", ["host", "device"])
def test_a_host_reader_that_throws(exe, stopping, tmp_path, tokens):  # noqa: F811
    """the same error on stderr, the same exit status and the same partial outputs as the default run"""
    files, at, pos = stopping
    outs = {}
    for tag, more in (("want", []), ("k1", ["--files-per-pass", "1"]), ("k3", ["--files-per-pass", "3"])):
        v, c, _, p = call(exe, files, tag, tmp_path, ["--batch-sites", "40", "--indel-tokens", tokens] + more, ok=False)
        outs[tag] = (p.returncode, [ln for ln in p.stderr.splitlines() if ln.startswith("[ERROR]")], open(v, "rb").read(), open(c, "rb").read())
    assert outs["want"][0] == 1 and len(outs["want"][1]) == 1
    assert outs["k1"] == outs["want"] and outs["k3"] == outs["want"]
    written = [int(ln.split(b"\t")[1]) for ln in outs["k1"][3].splitlines() if ln and not ln.startswith(b"#")]
    assert max(written) == pos - 1


def test_what_the_flag_refuses_and_notes(exe, batchfiles, cohorts, tmp_path):  # noqa: F811
    files, groups = batchfiles(3, 1)
    want = call(exe, files, "want", tmp_path)
    got = call(exe, files, "got", tmp_path, ["--files-per-pass", "2", "--inflate", "device", "--gpus", "2", "--device", "0"])
    same_outputs(want, got, False)
    assert "[NOTE] --files-per-pass runs on one engine" in got[3].stderr and "[NOTE] --files-per-pass reads and inflates on the host" in got[3].stderr
    assert got[2]["engines"] == 1 and "inflate" not in got[2]
    p = call(exe, files, "regions", tmp_path, ["--files-per-pass", "2", "--regions", "chr1:1000-1100"], ok=False)[3]
    assert p.returncode == 1 and "[ERROR] --files-per-pass with --regions is not built" in p.stderr
    fasta, bams, ids = cohorts(3)
    p = subprocess.run([exe, "-I", bams[0], "-R", fasta, "-r", REGION, "--files-per-pass", "2", "--output-vcf", str(tmp_path / "b.vcf"), "--output-cvg",
                        str(tmp_path / "b.cvg")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 1 and "[ERROR] --files-per-pass applies to batchfile input" in p.stderr


def test_more_batchfiles_than_descriptors(exe, batchfiles, tmp_path):  # noqa: F811
    """130 batchfiles, and a soft RLIMIT_NOFILE of 130 in the child: beside stdio that cannot hold a reader per file"""
    files, groups = batchfiles(130, 1)
    assert len(files) == 130
    want = call(exe, files, "want", tmp_path)  # (no limit)
    p = call(exe, files, "limited", tmp_path, ok=False, limit=len(files))[3]
    assert p.returncode != 0 and "open failure" in p.stderr, p.stderr[-1000:]  # the limit bites: the default route cannot open its files
    got = call(exe, files, "got", tmp_path, ["--files-per-pass", "4"], limit=len(files))
    same_outputs(want, got, False)
    check_counters(got, 4, 130)
