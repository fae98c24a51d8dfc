"""What the tests of the BGZF-member pileup share (bv_engine_pileup_bgzf, basevar_amd/host/raw_members.hpp): the stand-alone
harness tests/cpp/bam_members_check.cpp, which plans a window's fetches as compressed members and cut points and holds the plan
to BamFile::next_raw through basevar_amd/csrc/bv_pileup_core.h; the corpora it runs over; and the parse of what it writes."""
import os
import re
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bai_py  # noqa: E402
import bam_py  # noqa: E402
import pileup_ref as pr  # noqa: E402

SRC = os.path.join(ROOT, "tests", "cpp", "bam_members_check.cpp")
DEPS = pr.DEPS + [SRC, os.path.join(ROOT, "basevar_amd", "host", "raw_members.hpp"), os.path.join(ROOT, "basevar_amd", "host", "raw_reads.hpp")]
RUN_DTYPE = np.dtype([("sample", "<u4"), ("first_member", "<u4"), ("n_members", "<u4"), ("begin", "<u4"), ("end", "<u4"), ("reserved_", "<u4")])
COUNTS = ("members", "runs", "begin_gt0", "end_lt_isize", "chunk_end_low0", "straddle", "span3", "multi_run", "shared", "no_run", "isize0")
RANGE_BAM = os.path.join(ROOT, "tests", "golden", "data", "range.bam")


def build(asan=False):
    """The harness: plain, or with ASan + UBSan (a program of its own: it needs no preloaded runtime)."""
    exe = os.path.join(pr.OUT_DIR, "bam_members_check" + (".asan" if asan else ""))
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in DEPS):
        return exe
    os.makedirs(pr.OUT_DIR, exist_ok=True)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-fno-omit-frame-pointer"] if asan else ["-O1"]
    tmp = exe + ".%d.tmp" % os.getpid()
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include")] + flags + [SRC, "-lz", "-o", tmp])
    os.replace(tmp, exe)
    return exe


class Plan:
    pass


def parse_members(path):
    b = open(path, "rb").read()
    assert b[:4] == b"PMEM"
    p = Plan()
    n_members, n_runs, p.tid, _, data_bytes = struct.unpack_from("<IIiIQ", b, 4)
    o = 4 + struct.calcsize("<IIiIQ")
    p.member_off = np.frombuffer(b, "<u8", n_members + 1, o).copy(); o += 8 * (n_members + 1)
    p.runs = np.frombuffer(b, RUN_DTYPE, n_runs, o).copy(); o += 24 * n_runs
    p.data = np.frombuffer(b, np.uint8, data_bytes, o).copy(); o += data_bytes
    assert o == len(b)
    p.isize = np.array([int.from_bytes(p.data[int(e) - 4:int(e)].tobytes(), "little") for e in p.member_off[1:]], np.uint64)
    return p


def run_plan(exe, out, fasta, bams, window, ref_id=pr.REF_ID, region=pr.REGION, mapq_thd=pr.MAPQ_THD):
    """the harness over the files: (pileup_ref Dump of the next_raw route, Plan, counts dict); raises if plan and next_raw differ"""
    cmd = [exe, "plan", str(out), fasta, ref_id, str(region[0]), str(region[1]), str(window[0]), str(window[1]), str(mapq_thd)] + list(bams)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("bam_members_check: exit %d\n%s\n%s" % (p.returncode, p.stdout.decode(), p.stderr.decode()[-3000:]))
    text = p.stdout.decode()
    m = re.search(r"^plan " + " ".join(k + r" (\d+)" for k in COUNTS) + "$", text, re.M)
    assert m, text
    return pr.parse(out), parse_members(str(out) + ".members"), dict(zip(COUNTS, map(int, m.groups())))


# ------------------------------------------------------------------------------------------------------------------ the corpora
class Corpus:
    """pileup_ref's seeded samples (sample 0 the special one, every seventh from 3 without reads) as BAM files of one block size,
    with or without an index; `lead_empty`: that many leading samples without reads"""

    def __init__(self, directory, n, block_payload, indexed, seed=20, lead_empty=0):
        os.makedirs(str(directory), exist_ok=True)
        self.fa = pr.reference()
        self.fasta = os.path.join(str(directory), "ref.fa")
        pr.write_fasta(self.fasta, self.fa)
        self.bams, self.recs = [], []
        for s in range(n):
            rng = np.random.default_rng(seed + s)
            recs = pr.special_sample(rng) if s == 0 else pr.random_sample(rng)
            if (s and s % 7 == 3) or s < lead_empty:
                recs = []
            path = os.path.join(str(directory), "s%03d.bam" % s)
            bam_py.write_bam(path, pr.REFS, recs, block_payload=block_payload)
            if indexed:
                bai_py.write_bai(path)
            self.bams.append(path)
            self.recs.append(recs)


SHARED_WINDOW = (40000, 40063)


def shared_member_sample(rng, k=0):
    """Two chunks of one fetch that meet inside one BGZF member: a long record (an N operation) reaches into the window from far
    left and lies in a wide bin; short records that end before the window follow it in a leaf bin the fetch does not want; then
    come the window's reads in the window's leaf bin.  At 700 bytes a member the three groups share members."""
    r = [pr.read(rng, 100 + k, [(pr.M, 20), (pr.N, 39900), (pr.M, 30)])]
    r += [pr.read(rng, 200 + 10 * i + k, [(pr.M, 25)]) for i in range(3)]
    r += [pr.read(rng, p + k, [(pr.M, 40), (pr.I, 2), (pr.M, 30)]) for p in range(39900, 40100, 17)]
    return r


def aligned_sample(rng, block_payload):
    """reads of SHARED_WINDOW whose last record ends exactly where a member of `block_payload` bytes ends: with bai_py's choice of
    virtual offsets the last chunk's end has a zero low half"""
    recs = [pr.read(rng, p, [(pr.M, 50)]) for p in range(39950, 40080, 13)]
    header = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in pr.REFS) + "@RG\tID:x\tSM:synth\n"
    size = 4 + 4 + len(header.encode()) + 4 + sum(4 + len(n) + 1 + 4 for n, _ in pr.REFS) + sum(len(pr.record_bytes(r)) for r in recs)
    pad = (-size) % block_payload  # longer read names fill the stream up (a name holds at most 254 letters)
    for r in recs:
        take = min(pad, 200)
        r["name"] = "r" + "x" * take
        pad -= take
    assert pad == 0
    return recs


def write_special(directory, block_payload=700):
    """-> (bams, fasta, fa): two shared-member samples and one aligned sample, indexed"""
    os.makedirs(str(directory), exist_ok=True)
    fa = pr.reference()
    fasta = os.path.join(str(directory), "ref.fa")
    pr.write_fasta(fasta, fa)
    rng = np.random.default_rng(77)
    bams = []
    for s, recs in enumerate([shared_member_sample(rng), shared_member_sample(rng, 3), aligned_sample(rng, block_payload)]):
        path = os.path.join(str(directory), "x%d.bam" % s)
        bam_py.write_bam(path, pr.REFS, recs, block_payload=block_payload)
        bai_py.write_bai(path)
        bams.append(path)
    return bams, fasta, fa
