"""CPU tests (no GPU) of the file-major batchfile reader behind `bv_call --files-per-pass` (basevar_amd/host/file_major.hpp):
tests/cpp/text_job_check.cpp, a program of its own built with AddressSanitizer and UBSan, drives it over a small cohort's
batchfiles -- written by `bv_pileup --rows host -B N` -- and holds the groups' rows, joined again, to the rows the default
producer's run_text delivers, for K = 1, 2, F - 1, F, F + 3 files per pass and windows of 1, 2, 65 and all positions; files of
unequal length end at the shortest; never more than K batchfiles are open.  And the header declares what _capi binds."""
import gzip
import os
import re
import struct
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pileup_ref as pr  # noqa: E402
from test_gpu_pileup_call import cohort  # noqa: E402
from test_pileup_batches_cpu import batch_names  # noqa: E402

BV_PILEUP = os.path.join(ROOT, "basevar_amd", "lib", "bv_pileup")
SRC = os.path.join(ROOT, "tests", "cpp", "text_job_check.cpp")
OUT_DIR = os.path.join(ROOT, "basevar_amd", "lib", "san")
REGION = "chr1:900-1300"
N, B = 20, 3  # 7 batchfiles of 3, 3, 3, 3, 3, 3 and 2 samples


@pytest.fixture(scope="module")
def check_exe():
    exe = os.path.join(OUT_DIR, "text_job_check.asan")
    deps = [SRC] + [os.path.join(ROOT, "basevar_amd", "host", h) for h in ("file_major.hpp", "batch_producer.hpp", "batchfile_fast.hpp", "batchfile.hpp")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
        os.makedirs(OUT_DIR, exist_ok=True)
        tmp = exe + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "include"), SRC, "-lz", "-o", tmp])
        os.replace(tmp, exe)
    return exe


@pytest.fixture(scope="module")
def batchfiles(tmp_path_factory):
    import __graft_entry__ as g
    if not os.path.exists(BV_PILEUP):
        g.build()
    fasta, bams, ids = cohort(tmp_path_factory.mktemp("job_cohort"), N)
    prefix = str(tmp_path_factory.mktemp("job_batches") / "c")
    args = [BV_PILEUP, "-R", fasta, "--regions", REGION, "-q", str(pr.MAPQ_THD), "--thread", "4", "-o", prefix, "-B", str(B), "--rows", "host"]
    p = subprocess.run(args + sum((["-I", b] for b in bams), []), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = batch_names(prefix, N, B)
    assert len(names) == 7 and all(os.path.exists(n) for n in names)
    return names


def members(path):
    """[(file offset, inflated bytes)] of a BGZF file's members"""
    data, at, out = open(path, "rb").read(), 0, []
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 14] == b"BC"
        total = struct.unpack_from("<H", data, at + 16)[0] + 1
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        out.append((at, zlib.decompress(data[at + 12 + xlen:at + total - 8], -15)))
        at += total
    return out


def run(exe, files):
    p = subprocess.run([exe] + list(files), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    return p.stdout


def test_groups_rejoined_are_the_default_routes_rows(check_exe, batchfiles):
    # the corpus: window boundaries inside a BGZF member -- a row that is neither a member's first nor the file's first begins
    # every window of 1, and those of 2 and 65 positions too
    for W in (1, 2, 65):
        inside = 0
        for f in batchfiles:
            starts, at = set(), 0
            for off, text in members(f):
                starts.add(at)
                at += len(text)
            text = gzip.decompress(open(f, "rb").read())
            body = text.index(b"\n", text.rindex(b"\n#") + 1) + 1 if b"\n#" in text else 0  # behind the header
            line_at = [body]
            while text.find(b"\n", line_at[-1]) >= 0 and text.find(b"\n", line_at[-1]) + 1 < len(text):
                line_at.append(text.find(b"\n", line_at[-1]) + 1)
            assert len(line_at) > 130
            inside += sum(1 for k in range(W, len(line_at), W) if line_at[k] not in starts)
        assert inside > 0, W
    out = run(check_exe, batchfiles)
    rows = [ln.split() for ln in out.splitlines() if ln.startswith("K ")]
    assert {(int(r[1]), int(r[3])) for r in rows} == {(k, w) for k in (1, 2, 6, 7, 10) for w in (1, 2, 65, 1 << 30)}
    for r in rows:
        K, windows, passes, max_open = int(r[1]), int(r[7]), int(r[9]), int(r[11])
        assert 1 <= max_open <= K
        assert passes >= windows * ((7 + K - 1) // K)
    n_pos = int(out.split()[1])
    assert n_pos == 401  # chr1:900-1300
    assert any(int(r[7]) == 401 for r in rows) and any(int(r[7]) == 1 for r in rows)


def test_files_of_unequal_length_end_at_the_shortest(check_exe, batchfiles, tmp_path):
    """three files cut short -- in group 0, in a middle group and in the last, one of them in the middle of a window of 65 --
    written as plain text, plain gzip and BGZF (the reader's three kinds of cursor)"""
    files = list(batchfiles)
    for f, keep, kind in ((0, 300, "bgzf"), (3, 133, "plain"), (6, 200, "gzip")):
        text = gzip.decompress(open(batchfiles[f], "rb").read())
        lines = text.split(b"\n")
        n_head = sum(1 for ln in lines if ln.startswith(b"#"))
        cut = b"\n".join(lines[:n_head + keep]) + b"\n"
        path = str(tmp_path / ("short%d" % f))
        if kind == "plain":
            open(path, "wb").write(cut)
        elif kind == "gzip":
            open(path, "wb").write(gzip.compress(cut))
        else:  # members of 1,000 bytes: rows span them
            with open(path, "wb") as o:
                for at in range(0, len(cut), 1000):
                    raw = zlib.compressobj(6, zlib.DEFLATED, -15)
                    body = raw.compress(cut[at:at + 1000]) + raw.flush()
                    o.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body +
                            struct.pack("<II", zlib.crc32(cut[at:at + 1000]), len(cut[at:at + 1000])))
                o.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
        files[f] = path
    out = run(check_exe, files)
    assert int(out.split()[1]) == 133
    assert len([ln for ln in out.splitlines() if ln.startswith("K ")]) == 5 * 4 * 2


def test_header_declares_what_capi_binds():
    from basevar_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "basevar_amd_text_job.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(bv_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted(_capi.TEXT_JOB_EXPORTS) and len(declared) == 3
