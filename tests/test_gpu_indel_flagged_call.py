"""GPU tests of `bv_call --emit device` on a row the indel tally leaves to the caller (row_flag = 1: its column would exceed
BV_IT_COLUMN_MAX = 16,384 bytes): the row goes in as host text with a column the host makes from the row's tokens, which reach
the host by one of three routes -- the SiteTexts' strings (batchfile input), one lazy fetch of the engine's list (batchfile input
with --indel-tokens device) or one lazy fetch of the window's pileup tokens (BAM input).  Every run writes the default run's
bytes, `--timing` shows the row among indel_columns_host with no host-formatted record, and the list's fetch shows in
text_fetch_bytes.  Before the tool runs, each test feeds its input through the Python engine and asserts that the special
position is parsed on the device and that the tally flags it."""
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
from test_gpu_bgzf_call import as_bgzf  # noqa: E402
from test_gpu_record_text_call import call, same_outputs  # noqa: E402
from test_gpu_text_tokens_call import model  # noqa: E402
from test_gpu_vcf_emit_call import ARGS, exe  # noqa: E402,F401
from test_host_formats import make_batchfiles  # noqa: E402

COLUMN_MAX = 16384  # BV_IT_COLUMN_MAX
N_SAMPLES, N_FILES, N_SITES, AT = 300, 3, 9, 4  # the batchfile cohort; AT: the special position's index
PLAIN = 4  # samples of every file that carry a plain base at the special position (the CVG row's depth counts A, C, G, T only)


def column_bytes(tokens):
    """the size of indel_string's column: TOKEN|count of the distinct tokens, comma-separated"""
    count = {}
    for t in tokens:
        count[t] = count.get(t, 0) + 1
    return sum(len(t) + 1 + len(str(c)) for t, c in count.items()) + len(count) - 1


def rewrite(paths, directory, special):
    """the batchfiles with position AT's rows replaced by rows of distinct 62-byte insertions (special), or taken out"""
    per = N_SAMPLES // N_FILES
    rng = np.random.default_rng(5)
    out, tokens = [], []
    for f, p in enumerate(paths):
        lines = gzip.open(p, "rt").read().split("\n")
        at = next(k for k, ln in enumerate(lines) if not ln.startswith("#")) + AT
        if special:
            fld = lines[at].split("\t")
            bases = []
            for i in range(per):
                tag = "".join("ACGT"[((f * per + i) >> (2 * k)) & 3] for k in range(5))  # the sample's index: no two alike
                bases.append("ACGT"[i] if i < PLAIN else "+" + tag + "".join("ACGT"[x] for x in rng.integers(0, 4, 56)))
            tokens += bases[PLAIN:]
            fld[3:] = [str(per), " ".join(["60"] * per), " ".join(bases), " ".join(["I"] * per), " ".join(str(1 + i % 100) for i in range(per)),
                       " ".join("+-"[i % 2] for i in range(per))]
            lines[at] = "\t".join(fld)
        else:
            del lines[at]
        q = os.path.join(str(directory), ("flagged_%d.bf.gz" if special else "plain_%d.bf.gz") % f)
        with gzip.open(q, "wt") as fh:
            fh.write("\n".join(lines))
        out.append(q)
    return out, tokens


@pytest.fixture(scope="module")
def flagged_batchfiles(tmp_path_factory):
    d = tmp_path_factory.mktemp("flagged")
    paths, ids, _ = make_batchfiles(d, n_sites=N_SITES, n_samples=N_SAMPLES, n_files=N_FILES)
    with_row, tokens = rewrite(paths, d, True)
    without, _ = rewrite(paths, d, False)
    assert len(set(tokens)) == len(tokens) == N_SAMPLES - N_FILES * PLAIN and column_bytes(tokens) > COLUMN_MAX
    return with_row, as_bgzf(with_row), as_bgzf(without), tokens


def test_a_batchfile_row_beyond_the_tallys_domain(exe, flagged_batchfiles, tmp_path):  # noqa: F811
    import basevar_amd as bv
    from basevar_amd import _capi
    gz_files, files, without, tokens = flagged_batchfiles
    # the precondition: the device parses the special position, its list holds the position's tokens, and the tally flags its row
    rows = [[ln.encode() for ln in gzip.open(f, "rt").read().split("\n") if ln and not ln.startswith("#")] for f in gz_files]
    eng = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(N_SAMPLES), device=0, max_samples=N_SAMPLES)
    try:
        b = eng.lrt_text([list(r) for r in zip(*rows)], [N_SAMPLES // N_FILES] * N_FILES, tokens="device")
        assert b.positions.tolist() == list(range(N_SITES)) and not (b.row_state[:, 0] & (_capi.BV_TEXT_SKIP | _capi.BV_TEXT_HOST)).any()
        assert int((b.tokens["pos"] == AT).sum()) == len(tokens)
        col_off, flag = eng.indel_tally(b.positions, b.tokens, b.token_text)
        assert flag.tolist() == [1 if p == AT else 0 for p in range(N_SITES)] and col_off[AT + 1] == col_off[AT]
    finally:
        eng.close()
    m = model(files)
    assert m["token_bytes"] > COLUMN_MAX
    for inflate in ("host", "device"):
        base = ["--batchfiles", ",".join(files)] + ARGS + ["--thread", "4", "--batch-sites", "64", "--inflate", inflate]
        want = call(exe, base, "want_" + inflate, tmp_path)
        assert "indel_columns_host" not in want[2]
        for tag, more in (("emit", ["--emit", "device"]), ("list", ["--emit", "device", "--indel-tokens", "device"])):
            got = call(exe, base, tag + "_" + inflate, tmp_path, more)
            same_outputs(want, got, False)
            t = got[2]
            print(tag, inflate, {k: t.get(k) for k in ("indel_columns_host", "indel_columns_device", "lines_host_formatted", "text_fetch_bytes")})
            assert t["emit"] == "device" and t["indel_columns_host"] >= 1 and t["lines_host_formatted"] == 0
            assert "[NOTE]" not in got[3].stderr
        # the lazy fetch of the engine's list: the whole batch's list comes over for the one flagged row
        plain = call(exe, ["--batchfiles", ",".join(without)] + base[2:], "plain_" + inflate, tmp_path, ["--emit", "device", "--indel-tokens", "device"])
        print("without", inflate, plain[2].get("text_fetch_bytes"), "list", m["token_bytes"])
        assert plain[2]["indel_columns_host"] == 0
        assert got[2]["text_fetch_bytes"] >= plain[2]["text_fetch_bytes"] + m["token_bytes"]


ANCHOR = 1800  # 1-based; the insertions' reads begin at its 0-based twin, so their anchor is this position
N_INDEL, N_PLAIN, INS = 70, 4, 250


def flagged_bams(directory):
    """N_PLAIN files of one read of plain bases across the anchor, then N_INDEL files of one `I250 M12` read each: an insertion
    of the file's own at the anchor"""
    fa = pr.reference()
    fasta = os.path.join(str(directory), "ref.fa")
    pr.write_fasta(fasta, fa)
    paths, recs_of = [], []
    for f in range(N_PLAIN + N_INDEL):
        rng = np.random.default_rng(900 + f)
        recs = [pr.read(rng, ANCHOR - 20, [(pr.M, 40)])] if f < N_PLAIN else [pr.read(rng, ANCHOR, [(pr.I, INS), (pr.M, 12)])]
        header = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in pr.REFS) + "@RG\tID:x\tSM:flag%02d\n" % f
        path = os.path.join(str(directory), "flag%02d.bam" % f)
        bam_py.write_bam(path, pr.REFS, recs, header_text=header, block_payload=700)
        paths.append(path)
        recs_of.append(recs)
    tokens = ["+" + fa[ANCHOR - 1] + r[0]["seq"][:INS] for r in recs_of[N_PLAIN:]]
    assert len(set(tokens)) == N_INDEL and column_bytes(tokens) > COLUMN_MAX
    return fa, fasta, paths, recs_of


def test_a_pileup_row_beyond_the_tallys_domain(exe, tmp_path):  # noqa: F811
    from test_gpu_pileup_bgzf import engine
    fa, fasta, bams, recs_of = flagged_bams(tmp_path)
    n, window = len(bams), (ANCHOR - 30, ANCHOR + 30)
    # the precondition: the pileup takes the reads, and the tally over its tokens flags the anchor's row
    runs = [b"".join(pr.record_bytes(r) for r in recs) for recs in recs_of]
    run_off = np.zeros(n + 1, np.uint64)
    run_off[1:] = np.cumsum([len(r) for r in runs])
    e = engine(fa, max_sites=300, n=n)
    try:
        n_cov = e.pileup(b"".join(runs), run_off, np.arange(n, dtype=np.uint32), n, pr.TID, window, window, pr.MAPQ_THD)
        _, pos, depth = e.pileup_rows()
        assert n_cov == 40 and ANCHOR in pos.tolist()
        col_off, flag = e.indel_tally(pos)
        assert flag.tolist() == [1 if p == ANCHOR else 0 for p in pos.tolist()]
        got = e.pileup_fetch()
        assert int((got["tokens"]["pos"] == ANCHOR).sum()) == N_INDEL
    finally:
        e.close()
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", "chr1:%d-%d" % window, "-q", str(pr.MAPQ_THD), "--thread", "4", "--batch-sites", "300"]
    want = call(exe, args, "host", tmp_path)
    for inflate in ("host", "device"):
        got = call(exe, args, "dev_" + inflate, tmp_path, ["--pileup", "device", "--emit", "device", "--inflate", inflate])
        same_outputs(want, got, False)
        t = got[2]
        print(inflate, {k: t.get(k) for k in ("indel_columns_host", "indel_columns_device", "lines_host_formatted", "cvg_lines_device")})
        assert t["emit"] == "device" and t["pileup"] == "device" and t["indel_columns_host"] >= 1 and t["lines_host_formatted"] == 0
        assert "[NOTE]" not in got[3].stderr
    assert open(want[1], "rb").read().count(b"|1,+") >= N_INDEL - 1  # the anchor's row is there, with its column
