"""GPU tests (-m gpu) of the batchfile text-row path (bv_engine_text_parse / bv_engine_text_submit, BaseTypeEngine.lrt_text):
seeded slabs written out as the reference's own batchfile rows must come back as the records of lrt() on the slab, byte for
byte, with the cell / phred planes of the slab, and with every position parsed on the device; positions whose Depth fields sum
to 0 give no record; and tests/cpp/text_rows_check.cpp holds the device against the host reader on valid, odd and damaged rows."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from basevar_amd.synth import make_slab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digits(v, width):
    """decimal tokens of the integer array v (< 10**width): (bytes [.., width], lengths)"""
    v = v.astype(np.int64)
    L = np.ones(v.shape, np.int64)
    for k in range(1, width):
        L += v >= 10 ** k
    out = np.zeros(v.shape + (width,), np.uint8)
    for j in range(width):
        k = np.maximum(L - 1 - j, 0)
        out[..., j] = 48 + (v // 10 ** k) % 10
    return out, L


def slab_rows(slab, file_samples, depth_zero=()):
    """The slab as batchfile text: (text uint8, row_off uint64 [P * F + 1]), built with numpy byte operations.  Cells:
    0-3 (+4 reverse) A C G T with strand + / -, 8 N with strand '.', 9 / 10 the indel tokens "+A" / "-C".  Depth is the
    number of covered samples of the file (0 for the positions in depth_zero)."""
    bs = np.asarray(slab["base_strand"])
    P, N = bs.shape[0], int(slab["n_samples"])
    bs = bs[:, :N]
    fs = np.asarray(file_samples, np.int64)
    F = fs.size
    foff = np.concatenate([[0], np.cumsum(fs)[:-1]])
    fid = np.repeat(np.arange(F), fs)
    cols = []
    tok, L = digits(np.asarray(slab["mapq"])[:, :N], 3)
    cols.append((tok, L))
    base = np.zeros((P, N, 2), np.uint8)
    base[..., 0] = np.frombuffer(b"ACGT", np.uint8)[bs & 3]
    base[..., 0] = np.where(bs == 8, ord("N"), np.where(bs == 9, ord("+"), np.where(bs == 10, ord("-"), base[..., 0])))
    base[..., 1] = np.where(bs == 9, ord("A"), ord("C"))
    cols.append((base, np.where(bs >= 9, 2, 1)))
    cols.append(((np.asarray(slab["qual"])[:, :N] + 33).astype(np.uint8)[..., None], np.ones((P, N), np.int64)))
    cols.append(digits(np.asarray(slab["rpr"])[:, :N], 5))
    strand = np.where(bs >= 8, ord("."), np.where(bs & 4, ord("-"), ord("+"))).astype(np.uint8)
    cols.append((strand[..., None], np.ones((P, N), np.int64)))
    covered = np.add.reduceat((bs != 8).astype(np.int64), foff, axis=1)  # [P, F]
    covered[list(depth_zero), :] = 0
    ref = np.frombuffer(b"ACGTN", np.uint8)[np.minimum(np.asarray(slab["ref_base"]), 4)]
    prefix = [[b"chr9\t%d\t%s\t%d\t" % (1000 + p, bytes([ref[p]]), covered[p, f]) for f in range(F)] for p in range(P)]
    plen = np.array([[len(x) for x in r] for r in prefix], np.int64)
    lens = [L + 1 for _, L in cols]  # every token and the separator behind it
    colsum = [np.add.reduceat(l, foff, axis=1) for l in lens]  # [P, F]
    rowlen = plen + sum(colsum)
    row_off = np.zeros(P * F + 1, np.uint64)
    row_off[1:] = np.cumsum(rowlen.reshape(-1))
    text = np.zeros(int(row_off[-1]), np.uint8)
    rstart = row_off[:-1].astype(np.int64).reshape(P, F)
    for p in range(P):
        for f in range(F):
            text[rstart[p, f]:rstart[p, f] + plen[p, f]] = np.frombuffer(prefix[p][f], np.uint8)
    col_at = rstart + plen
    last = np.zeros(N, bool)
    last[np.cumsum(fs) - 1] = True
    for c, ((tok, L), l) in enumerate(zip(cols, lens)):
        ex = np.cumsum(l, axis=1) - l
        ex = ex - ex[:, foff][:, fid]  # inside the file's segment
        at = col_at[:, fid] + ex  # [P, N]
        for j in range(tok.shape[-1]):
            m = L > j
            text[at[m] + j] = tok[..., j][m]
        sep = np.where(last, ord("\n") if c == 4 else ord("\t"), ord(" ")).astype(np.uint8)
        text[at + L] = np.broadcast_to(sep, at.shape)
        col_at = col_at + colsum[c]
    return text, row_off


def run(slab, file_samples, n_groups=0, depth_zero=()):
    import basevar_amd as bv
    N = int(slab["n_samples"])
    P = slab["base_strand"].shape[0]
    eng = bv.BaseTypeEngine(max_sites=P, min_af_value=bv.min_af(N), device=0, max_samples=N)
    try:
        gid = slab.get("group_id") if n_groups else None
        got = eng.lrt_text(slab_rows(slab, file_samples, depth_zero), file_samples, group_id=gid, n_groups=n_groups)
        keep = np.array([p for p in range(P) if p not in set(depth_zero) and (slab["base_strand"][p, :N] != 8).any()], np.int64)
        sub = {k: (v[keep] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == P and k != "group_id" else v)
               for k, v in slab.items()}
        exp = eng.lrt(sub)
    finally:
        eng.close()
    return got, exp, keep


def check(slab, file_samples, n_groups=0, depth_zero=()):
    from basevar_amd import _capi
    got, exp, keep = run(slab, file_samples, n_groups, depth_zero)
    N = int(slab["n_samples"])
    assert not (got.row_state & _capi.BV_TEXT_HOST).any(), "a well-formed position went to the host reader"
    assert np.array_equal(got.positions, keep)
    assert got.sites.tobytes() == exp.sites.tobytes(), [f for f in got.sites.dtype.names
                                                        if not np.array_equal(got.sites[f], exp.sites[f], equal_nan=got.sites[f].dtype.kind == "f")]
    if n_groups:
        assert got.groups.tobytes() == exp.groups.tobytes()
    assert got.n_variant == exp.n_variant
    assert np.array_equal(got.cell, slab["base_strand"][keep, :N])
    assert np.array_equal(got.phred, slab["qual"][keep, :N])
    return got


def test_one_file_of_60_samples():
    slab = make_slab(96, 60, seed=301, coverage=0.3, indel_frac=0.05)
    got = check(slab, [60])
    assert got.n_variant > 0


def test_seven_files_of_200_and_one_of_37_with_groups_and_long_reads():
    slab = make_slab(40, 7 * 200 + 37, seed=302, coverage=0.1, indel_frac=0.02, n_groups=2)
    check(slab, [200] * 7 + [37], n_groups=2)  # ranks <= 100: the tagged layout
    slab["rpr"][5, :50] = np.where(slab["base_strand"][5, :50] != 8, 9000 + np.arange(50), 0)  # one read beyond 8,191: plain
    check(slab, [200] * 7 + [37], n_groups=2)


def test_ten_thousand_samples_in_files_of_200():
    slab = make_slab(24, 10000, seed=303, coverage=0.08)
    assert check(slab, [200] * 50).n_variant > 0


def test_a_million_samples_in_5000_files():
    slab = make_slab(16, 1_000_000, seed=304, coverage=0.02, indel_frac=0.002)
    check(slab, [200] * 5000)


def test_depth_zero_positions_give_no_record():
    slab = make_slab(32, 400, seed=305, coverage=0.1)
    slab["base_strand"][[3, 17], :] = 8  # all-N files: Depth 0 everywhere
    for k in ("qual", "mapq", "rpr"):
        slab[k][[3, 17], :] = 0
    got = check(slab, [200, 200], depth_zero=(9, 25))  # covered cells, but Depth fields of 0: skipped as the host reader does
    from basevar_amd import _capi
    assert (got.row_state[[3, 9, 17, 25]] == _capi.BV_TEXT_SKIP).all()


def build_text_rows_check(tmp_path):
    exe = tmp_path / "text_rows_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "text_rows_check.cpp"), "-L", os.path.join(ROOT, "basevar_amd", "lib"),
                           "-lbasevar_amd", "-Wl,-rpath," + os.path.join(ROOT, "basevar_amd", "lib"), "-o", str(exe)])
    return str(exe)


def test_device_parser_against_the_host_reader(tmp_path):
    exe = build_text_rows_check(tmp_path)
    p = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "FAILS 0" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_device_parser_on_the_positional_corpus(tmp_path):
    """tests/cpp/row_lane_cases.hpp through the device parser: valid rows of 3 to 10 of the kernel's 64-byte steps with every
    token start, tab and line break on every lane, and damaged rows whose defect sits on lanes 0, 1, 62, 63 and 31 of a step
    behind the first (the tracer's LANE_COVERAGE line says what was reached; anything missing is a failure).  Many positions to a
    batch: records, cell / phred planes, SiteText, positions kept and used and the error text are the host reader's, every valid
    and every clean row is parsed on the device, and all four outcomes occur.
    Measured on an MI355X in one run, compiling the harness included: test_device_parser_against_the_host_reader (as in the parent
    commit; the library is the parent's) 3.74 s, this test 3.30 s (194 batches); test_gpu_bgzf_rows.py's corpus test 5.07 s as
    the first test of its process, its line-index tests 0.01 to 0.04 s each."""
    import re
    exe = build_text_rows_check(tmp_path)
    p = subprocess.run([exe, "0", "lanes"], capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "FAILS 0" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert re.search(r"LANE_COVERAGE rows \d+ .* missing 0\n", p.stdout) and re.search(r"LANE_CASES .* bad 0\n", p.stdout), p.stdout[-3000:]
    m = re.search(r"TEXT_ROWS_LANES batches (\d+) device (\d+) host (\d+) skipped (\d+) threw (\d+)", p.stdout)
    assert m and all(int(g) > 0 for g in m.groups()), p.stdout[-3000:]


def test_text_staging_reused_over_many_chunks(monkeypatch):
    """chunks of 64 KiB (BASEVAR_AMD_TEXT_CHUNK_BYTES): the two pinned and two device buffers are each reused ~10 times"""
    monkeypatch.setenv("BASEVAR_AMD_TEXT_CHUNK_BYTES", str(64 << 10))
    slab = make_slab(64, 2000, seed=306, coverage=0.2, indel_frac=0.02)
    text, _ = slab_rows(slab, [200] * 10)
    assert text.size > 20 * (64 << 10)
    check(slab, [200] * 10)


def _py_host_reader(n):
    """a host reader for the test's rows (every odd form they hold: signed integers); None when the Depth fields sum to 0"""
    def read(lines):
        cols = [l.split(b"\t") for l in lines]
        if sum(int(c[3]) for c in cols) == 0:
            return None
        tok = [sum((c[k].split(b" ") for c in cols), []) for k in range(4, 9)]
        cell = np.array([8 if b[:1] == b"N" else 9 if b[:1] == b"+" else 10 if b[:1] == b"-" else
                         b"ACGT".index(b[:1]) | (4 if s == b"-" else 0) for b, s in zip(tok[1], tok[4])], np.uint8)
        ref = b"ACGT".find(cols[0][2][:1].upper())
        return (cell, np.array([q[0] - 33 for q in tok[2]], np.uint8), np.array([int(x) for x in tok[0]], np.uint8),
                np.array([int(x) for x in tok[3]], np.uint16), 4 if ref < 0 else ref)
    return read


def test_host_positions_through_a_python_host_reader():
    """positions the device leaves to the host: read by `host_reader`, put in place; one the reader skips (its Depth fields
    '+0') comes back BV_TEXT_SKIP.  Records == lrt() on the slab without the skipped position."""
    import basevar_amd as bv
    from basevar_amd import _capi
    fs = [100, 100]
    slab = make_slab(12, 200, seed=307, coverage=0.2)
    text, off = slab_rows(slab, fs)
    rows = [[bytes(text[int(off[p * 2 + f]):int(off[p * 2 + f + 1]) - 1]) for f in range(2)] for p in range(12)]

    def sign_mapq(row):  # "+60": the host reader takes the sign, the device does not
        c = row.split(b"\t")
        c[4] = b" ".join(b"+" + t for t in c[4].split(b" "))
        return b"\t".join(c)
    rows[4] = [sign_mapq(r) for r in rows[4]]
    rows[7] = [b"\t".join(c[:3] + [b"+0"] + c[4:]) for c in (r.split(b"\t") for r in rows[7])]
    eng = bv.BaseTypeEngine(max_sites=12, min_af_value=bv.min_af(200), device=0, max_samples=200)
    try:
        got = eng.lrt_text(rows, fs, host_reader=_py_host_reader(200))
        keep = np.array([p for p in range(12) if p != 7], np.int64)
        exp = eng.lrt({k: (v[keep] if isinstance(v, np.ndarray) and v.shape[0] == 12 else v) for k, v in slab.items()})
        # refusals on a live engine: NULL rows, a submit without a parse
        state = np.zeros(2, np.uint8)
        assert eng._lib.bv_engine_text_parse(eng._h, None, None, 0, state.ctypes.data, None) == _capi.BV_ERR_INVALID_ARG
        out = np.zeros(1, dtype=_capi.SITE_DTYPE)
        assert eng._lib.bv_engine_text_submit(eng._h, None, None, 1, out.ctypes.data, None, None, None, None) == _capi.BV_ERR_INVALID_ARG
        assert "no bv_engine_text_parse" in eng._err()
        with pytest.raises(RuntimeError, match="no host_reader"):
            eng.lrt_text(rows, fs)
    finally:
        eng.close()
    assert (got.row_state[4] == _capi.BV_TEXT_HOST).all() and (got.row_state[7] == _capi.BV_TEXT_SKIP).all()
    assert not (got.row_state[np.r_[0:4, 5:7, 8:12]] & (_capi.BV_TEXT_HOST | _capi.BV_TEXT_SKIP)).any()
    assert np.array_equal(got.positions, keep)
    assert got.sites.tobytes() == exp.sites.tobytes()
    assert np.array_equal(got.cell, slab["base_strand"][keep, :200]) and np.array_equal(got.phred, slab["qual"][keep, :200])


# ---- bv_call on batchfiles: the rows now go to the engines as text
def _bv_call(tmp_path):
    from test_host_formats import cxx
    return cxx(os.path.join(ROOT, "basevar_amd", "host", "bv_call.cpp"), str(tmp_path / "bv_call"), ["-lz"])


def _body(path):
    return [l for l in open(path).read().split("\n") if l and not l.startswith("#")]


def test_bv_call_damaged_row_inside_a_batch(tmp_path):
    """(c) a malformed row in the middle of a batch: the host reader's error text and exit status, and the CVG / VCF lines of
    the clean run up to that position"""
    import gzip
    from test_host_formats import _write_batchfiles
    exe = _bv_call(tmp_path)
    d = tmp_path / "bf"; d.mkdir()
    files = _write_batchfiles(str(d), 3, 40, 400, seed=21, bgzf=False)
    args = ["--batch-sites", "1000", "--contig", "chr1:1000", "--reference", "x.fa"]
    clean = subprocess.run([exe, "--batchfiles", ",".join(files), "--output-vcf", str(tmp_path / "a.vcf"), "--output-cvg",
                            str(tmp_path / "a.cvg")] + args, capture_output=True, text=True, timeout=300)
    assert clean.returncode == 0, clean.stderr
    lines = gzip.open(files[1], "rb").read().decode().split("\n")
    cols = lines[3 + 250].split("\t")  # position 350 (row 251) of file 1: a two-letter base token on a covered sample
    k = next(i for i, s in enumerate(cols[8].split(" ")) if s in "+-")
    toks = cols[5].split(" "); toks[k] = "AC"; cols[5] = " ".join(toks)
    lines[3 + 250] = "\t".join(cols)
    gzip.open(files[1], "wb").write("\n".join(lines).encode())
    bad = subprocess.run([exe, "--batchfiles", ",".join(files), "--output-vcf", str(tmp_path / "b.vcf"), "--output-cvg",
                          str(tmp_path / "b.cvg")] + args, capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1, (bad.returncode, bad.stderr)
    assert "[ERROR] Why dose the size of aligned base is not 1? Check: AC" in bad.stderr
    before = lambda ls: [l for l in ls if int(l.split("\t")[1]) < 350]
    assert _body(tmp_path / "b.cvg") == before(_body(tmp_path / "a.cvg")) and len(_body(tmp_path / "b.cvg")) > 200
    assert _body(tmp_path / "b.vcf") == before(_body(tmp_path / "a.vcf"))


def test_bv_call_engines_and_threads_write_the_same_bytes(tmp_path, restatement):
    """(d) --gpus 2 --devices 0,0 and --thread 1 / 7 write byte-identical files; every line is the reference caller's where its
    library is built"""
    from test_host_formats import make_batchfiles, reference_caller_lines
    exe = _bv_call(tmp_path)
    paths, ids, sites = make_batchfiles(tmp_path, n_sites=300, n_samples=60)
    outs = []
    for tag, extra in (("t1", ["--thread", "1"]), ("t7", ["--thread", "7", "--batch-sites", "13"]),
                       ("g2", ["--gpus", "2", "--devices", "0,0", "--thread", "4", "--batch-sites", "29"])):
        v, c = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".cvg"))
        p = subprocess.run([exe, "--batchfiles", ",".join(paths), "--output-vcf", v, "--output-cvg", c, "--contig", "chr17:81195210",
                            "--reference", "hg19.fa"] + extra, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        outs.append((open(v, "rb").read(), open(c, "rb").read()))
    assert outs[0] == outs[1] == outs[2]
    ref = reference_caller_lines(paths, 60, restatement.min_af(60, 0.01))
    if ref is not None:
        got_cvg, got_vcf = _body(tmp_path / "t1.cvg"), _body(tmp_path / "t1.vcf")
        assert got_cvg == ref[0] and len(got_vcf) == len(ref[1]) and len(got_vcf) > 0
