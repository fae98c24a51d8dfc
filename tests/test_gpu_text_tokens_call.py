"""GPU tests of `bv_call --indel-tokens device` (the '+SEQ' / '-SEQ' tokens of batchfile rows listed on the worker's engine,
include/basevar_amd_text_tokens.h): under --inflate host|device x --emit host|device, with and without pop-groups, VCF and CVG
are the bytes of the same run without the flag; --timing's indel_tokens_device and text_fetch_bytes are what a model computes
from the batchfiles' text; a cohort with a damaged row puts a host-read position between device-parsed ones; and on BAM input
the flag prints its note and changes nothing."""
import gzip
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_bgzf_call import as_bgzf  # noqa: E402
from test_gpu_indel_tally_call import indel_rows  # noqa: E402
from test_gpu_pileup_call import cohort  # noqa: E402
from test_gpu_record_text_call import call, same_outputs  # noqa: E402
from test_gpu_vcf_emit_call import ARGS, exe, inputs  # noqa: E402,F401
from test_host_formats import make_batchfiles  # noqa: E402
import pileup_ref as pr  # noqa: E402

TOKEN_BYTES = 24  # sizeof(bv_pileup_token)


def model(files, host_positions=()):
    """What the batchfiles' text says of a run: the tokens the engines list (count, text bytes), and the bytes the workers'
    rows fetch and heads fetch bring back.  A position whose Depth fields sum to 0 is skipped; `host_positions` go to the host
    reader whole; every other position is parsed on the device."""
    rows = [[ln for ln in gzip.open(f, "rb").read().split(b"\n") if ln and not ln.startswith(b"#")] for f in files]
    P = len(rows[0])
    assert all(len(r) == P for r in rows)
    n_tok = n_text = rows_fetch = heads_fetch = 0
    for p in range(P):
        lines = [r[p] for r in rows]
        if sum(int(ln.split(b"\t")[3]) for ln in lines) == 0:
            continue
        if p in host_positions:
            rows_fetch += sum(len(ln) for ln in lines)
            heads_fetch += sum(len(ln) for ln in lines)
            continue
        head = len(b"\t".join(lines[0].split(b"\t")[:4])) + 1
        heads_fetch += head
        for f, ln in enumerate(lines):
            toks = [t for t in ln.split(b"\t")[5].split(b" ") if t[:1] in (b"+", b"-")]
            n_tok += len(toks)
            n_text += sum(len(t) for t in toks)
            rows_fetch += len(ln) if toks else head if f == 0 else 0
    return dict(tokens=n_tok, token_bytes=TOKEN_BYTES * n_tok + n_text, rows_fetch=rows_fetch, heads_fetch=heads_fetch)


def check_pair(want, got, m, inflate, emit, gz):
    same_outputs(want, got, gz)
    tw, tg = want[2], got[2]
    assert tg["indel_tokens"] == "device" and "indel_tokens" not in tw and "indel_tokens_device" not in tw
    assert tg["indel_tokens_device"] == m["tokens"] > 100
    # the bytes that came back: the rows (heads) fetch where the engine inflates, and the one token fetch of every batch where
    # the host formats the rows (with --emit device no row of these cohorts is beyond the tally's domain: nothing is fetched)
    assert tw["text_fetch_bytes"] == (m["rows_fetch"] if inflate == "device" else 0)
    assert tg["text_fetch_bytes"] == (m["heads_fetch"] if inflate == "device" else 0) + (m["token_bytes"] if emit == "host" else 0)
    if emit == "device":
        assert tg["indel_columns_device"] + tg["indel_columns_host"] == tw["indel_columns_device"] + tw["indel_columns_host"] == indel_rows(want[1]) >= 20
    assert "[NOTE]" not in got[3].stderr


@pytest.mark.parametrize("emit", ["host", "device"])
@pytest.mark.parametrize("inflate", ["host", "device"])
def test_batchfile_runs_write_the_default_runs_files(exe, inputs, tmp_path, inflate, emit):  # noqa: F811
    files, groups = inputs
    m = model(files)
    base = ["--batchfiles", ",".join(files)] + ARGS + ["--thread", "4", "--inflate", inflate, "--emit", emit]
    for tag, more, gz in (("b50", ["--batch-sites", "50"], False), ("grp", ["--pop-group", groups, "--batch-sites", "64"], True)):
        want = call(exe, base + more, tag + "_want", tmp_path, gz=gz)
        got = call(exe, base + more, tag + "_got", tmp_path, ["--indel-tokens", "device"], gz=gz)
        check_pair(want, got, m, inflate, emit, gz)
        assert (got[2].get("inflate") == "device") == (inflate == "device") and (got[2].get("emit") == "device") == (emit == "device")


@pytest.fixture(scope="module")
def damaged(tmp_path_factory):
    """120 positions x 60 samples in three BGZF batchfiles; file 1's row of one position has a signed MappingQuality token: the
    host reader takes it (istringstream >> int), the device does not, so the position is host-read -- and its '+' is no token"""
    d = tmp_path_factory.mktemp("damaged")
    paths, ids, _ = make_batchfiles(d, n_sites=120, n_samples=60, n_files=3)
    lines = gzip.open(paths[1], "rb").read().split(b"\n")
    first = next(k for k, ln in enumerate(lines) if not ln.startswith(b"#"))
    all_rows = [[ln for ln in gzip.open(p, "rb").read().split(b"\n") if ln and not ln.startswith(b"#")] for p in paths]
    has = lambda p: any(t[:1] in (b"+", b"-") for r in all_rows for t in r[p].split(b"\t")[5].split(b" "))  # noqa: E731
    at = next(p for p in range(5, 100) if has(p - 1) and has(p) and has(p + 1))
    f = lines[first + at].split(b"\t")
    f[4] = b"+" + f[4]
    lines[first + at] = b"\t".join(f)
    with gzip.open(paths[1], "wb") as fh:
        fh.write(b"\n".join(lines))
    return as_bgzf(paths), at


@pytest.mark.parametrize("emit", ["host", "device"])
@pytest.mark.parametrize("inflate", ["host", "device"])
def test_a_host_read_position_between_device_parsed_ones(exe, damaged, tmp_path, inflate, emit):  # noqa: F811
    files, at = damaged
    m, clean = model(files, host_positions=[at]), model(files)
    assert 0 < m["tokens"] < clean["tokens"]  # the host-read position's tokens are not the engine's
    base = ["--batchfiles", ",".join(files)] + ARGS + ["--thread", "4", "--batch-sites", "40", "--inflate", inflate, "--emit", emit]
    want = call(exe, base, "want", tmp_path)
    got = call(exe, base, "got", tmp_path, ["--indel-tokens", "device"])
    same_outputs(want, got, False)
    assert got[2]["indel_tokens_device"] == m["tokens"]
    assert want[2]["text_fetch_bytes"] == (m["rows_fetch"] if inflate == "device" else 0)
    assert got[2]["text_fetch_bytes"] == (m["heads_fetch"] if inflate == "device" else 0) + (m["token_bytes"] if emit == "host" else 0)
    if emit == "device":
        assert got[2]["indel_columns_device"] + got[2]["indel_columns_host"] == want[2]["indel_columns_device"] + want[2]["indel_columns_host"] == indel_rows(want[1])
        assert got[2]["indel_columns_host"] >= 1  # the host-read row's column is the host's


def test_bam_input_prints_the_note_and_writes_the_default_files(exe, tmp_path):  # noqa: F811
    fasta, bams, ids = cohort(tmp_path, 3)
    args = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", "chr1:900-2300", "-q", str(pr.MAPQ_THD), "--thread", "2", "--batch-sites", "300"]
    want = call(exe, args, "want", tmp_path)
    got = call(exe, args, "got", tmp_path, ["--indel-tokens", "device"])
    same_outputs(want, got, False)
    assert "[NOTE] --indel-tokens device applies to batchfile input" in got[3].stderr and "[NOTE]" not in want[3].stderr
    assert "indel_tokens" not in got[2] and "text_fetch_bytes" not in got[2]


@pytest.fixture(scope="module")
def stopping(tmp_path_factory):
    """120 positions x 60 samples in three BGZF batchfiles; file 1's row of one position, in the middle of a batch of 40, has a
    two-letter base token: the device leaves the position to the host reader, and the host reader throws -- it stops there, so
    that n_positions_used < P, with marked device-parsed positions before and behind it in the same batch"""
    d = tmp_path_factory.mktemp("stopping")
    paths, ids, _ = make_batchfiles(d, n_sites=120, n_samples=60, n_files=3)
    lines = gzip.open(paths[1], "rb").read().split(b"\n")
    first = next(k for k, ln in enumerate(lines) if not ln.startswith(b"#"))
    all_rows = [[ln for ln in gzip.open(p, "rb").read().split(b"\n") if ln and not ln.startswith(b"#")] for p in paths]
    has = lambda p: any(t[:1] in (b"+", b"-") for r in all_rows for t in r[p].split(b"\t")[5].split(b" "))  # noqa: E731
    at = next(p for p in range(48, 72) if has(p - 1) and has(p + 1) and has(p + 2))
    f = lines[first + at].split(b"\t")
    f[5] = b"AC" + f[5][f[5].index(b" "):]
    lines[first + at] = b"\t".join(f)
    with gzip.open(paths[1], "wb") as fh:
        fh.write(b"\n".join(lines))
    return as_bgzf(paths), at, int(all_rows[0][at].split(b"\t")[1])


@pytest.mark.parametrize("emit", ["host", "device"])
@pytest.mark.parametrize("inflate", ["host", "device"])
def test_a_host_reader_that_stops_at_a_position(exe, stopping, tmp_path, inflate, emit):  # noqa: F811
    """the run ends with the host reader's error behind the records before the position, with and without the flag alike: the
    tokens the engine listed for the positions behind the stop reach no record and no tally"""
    import subprocess
    files, at, pos = stopping
    outs = {}
    for tag, more in (("want", []), ("got", ["--indel-tokens", "device"])):
        v, c = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".cvg"))
        p = subprocess.run([exe, "--batchfiles", ",".join(files)] + ARGS + ["--thread", "4", "--batch-sites", "40", "--inflate", inflate, "--emit", emit,
                                                                          "--output-vcf", v, "--output-cvg", c] + more, capture_output=True, text=True, timeout=600)
        outs[tag] = (p.returncode, [ln for ln in p.stderr.splitlines() if ln.startswith("[ERROR]")], open(v, "rb").read(), open(c, "rb").read())
    # (the host reader's own message for the row: the strand check of the refused token comes before the base token's)
    assert outs["want"][0] == 1 and len(outs["want"][1]) == 1 and ("strange strand symbol" in outs["want"][1][0] or "size of aligned base" in outs["want"][1][0])
    assert outs["got"] == outs["want"]
    rows = [ln.split(b"\t") for ln in outs["got"][3].splitlines() if ln and not ln.startswith(b"#")]
    written = [int(r[1]) for r in rows]
    assert pos - 1 in written and max(written) == pos - 1 and min(written) < pos - (at % 40)  # the batch's records before the stop, none behind it
    assert any(r[8] != b"." for r in rows if int(r[1]) >= pos - (at % 40))                    # ... with indel columns among them
