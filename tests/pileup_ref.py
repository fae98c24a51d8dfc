"""What the tests of bv_engine_pileup share: the stand-alone harness tests/cpp/pileup_core_check.cpp (the host pileup as it
is, held on the way against the serial form of basevar_amd/csrc/bv_pileup_core.h), a seeded corpus of BAM files written with
bam_py.write_bam, and the check of a dumped result against bam_py.pileup_sample, the independent derivation."""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_py  # noqa: E402

SRC = os.path.join(ROOT, "tests", "cpp", "pileup_core_check.cpp")
DEPS = [SRC, os.path.join(ROOT, "basevar_amd", "csrc", "bv_pileup_core.h"), os.path.join(ROOT, "basevar_amd", "host", "pileup.hpp"),
        os.path.join(ROOT, "basevar_amd", "host", "bamio.hpp"), os.path.join(ROOT, "basevar_amd", "host", "batchfile.hpp"),
        os.path.join(ROOT, "include", "basevar_amd.h")]
OUT_DIR = os.path.join(ROOT, "basevar_amd", "lib", "san")

REFS = [("chr0", 2000), ("chr1", 600000), ("chr2", 2000)]
REF_ID, TID = "chr1", 1
REGION = (1, 600000)
MAPQ_THD = 10
STEP = 500000
# (beg, end) of the windows the tests pile up: rows 1000, 1, 2, 64, 65, the last rows of the first step, the first of the second
WINDOWS = {"w1000": (1000, 1999), "w1": (1100, 1100), "w2": (1219, 1220), "w64": (1300, 1363), "w65": (1400, 1464),
           "edge": (499990, 500000), "next": (500001, 500064)}
M, I, D, N, S, H, P, EQ, X = range(9)

BV_PILEUP_OK, BAD_BLOCK, BAD_RUN, BAD_LENGTHS, BAD_QUERY, BAD_REF, BAD_BASE = range(7)
BAD_BASE_TEXT = "[ERROR] Why dose the size of aligned base is not 1? Check:  "
TOKEN_DTYPE = np.dtype([("pos", "<u4"), ("sample", "<u4"), ("text_off", "<u8"), ("text_len", "<u4"), ("reserved_", "<u4")])
assert TOKEN_DTYPE.itemsize == 24


def build(asan=False):
    """The harness: plain, or with ASan + UBSan (a program of its own: it needs no preloaded runtime)."""
    exe = os.path.join(OUT_DIR, "pileup_core_check" + (".asan" if asan else ""))
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in DEPS):
        return exe
    os.makedirs(OUT_DIR, exist_ok=True)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-fno-omit-frame-pointer"] if asan else ["-O1"]
    tmp = exe + ".%d.tmp" % os.getpid()
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include")] + flags + [SRC, "-lz", "-o", tmp])
    os.replace(tmp, exe)
    return exe


# ------------------------------------------------------------------------------------------------------------------- the corpus
def reference(seed=7):
    """chr1: 600,000 seeded bases, lower case here and there (the tokens keep the letter case), an N run"""
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, REFS[1][1])].copy()
    seq[1260:1285] |= 0x20
    seq[1500:1600] |= 0x20
    seq[499995:500010] |= 0x20
    seq[1650:1655] = ord("N")
    return seq.tobytes().decode()


def write_fasta(path, fa):
    rng = np.random.default_rng(1)
    with open(path, "w") as f:
        for (name, ln), seq in zip(REFS, ["".join("ACGT"[i] for i in rng.integers(0, 4, REFS[0][1])), fa,
                                          "".join("ACGT"[i] for i in rng.integers(0, 4, REFS[2][1]))]):
            f.write(">%s test\n" % name)
            for o in range(0, ln, 100):
                f.write(seq[o:o + 100] + "\n")


def read(rng, pos, cigar, tid=TID, mapq=60, flag=0, seq=None, qual=None):
    n = sum(ln for op, ln in cigar if op in (M, I, S, EQ, X))
    if seq is None:
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    if qual is None:
        qual = [int(x) for x in rng.integers(2, 42, len(seq))]
    return dict(tid=tid, pos=pos, mapq=mapq, flag=flag, cigar=cigar, seq=seq, qual=qual)


def special_sample(rng):
    """every case the issue names, around the windows of WINDOWS (positions 0-based, as BAM holds them)"""
    r = [read(rng, 100, [(M, 50)], tid=0), read(rng, 1500, [(M, 50)], tid=0)]  # another reference before the query's
    r += [
        read(rng, 900, [(M, 150)]),                            # begins before the window
        read(rng, 950, [(M, 120)], flag=16),                   # overlaps it, and the next one: the first wins
        read(rng, 960, [(M, 100)]),
        read(rng, 999, [(I, 2), (M, 30)]),                     # an indel whose anchor lies before the window
        read(rng, 1060, [(M, 30)], mapq=MAPQ_THD - 1),         # just below the threshold
        read(rng, 1062, [(M, 30)], mapq=MAPQ_THD),             # at it
        read(rng, 1099, [(S, 5), (I, 3), (M, 50)]),            # starts with I behind S: the indel does claim
        read(rng, 1160, [(M, 20)], flag=1024),                 # duplicate
        read(rng, 1160, [(M, 20)], flag=512),                  # QC fail
        read(rng, 1160, [(M, 20)], flag=4 | 1024),             # unmapped (and then "duplicate" does not count: still nothing)
        read(rng, 1165, [(M, 20)], flag=16),
        read(rng, 1200, [(S, 5), (I, 2), (D, 3), (M, 20)]),    # I then D at one break point: one anchor, the I holds it
        read(rng, 1225, [(M, 10), (I, 2), (M, 5), (D, 2), (M, 5)]),  # indels behind the read's own match: refused
        read(rng, 1250, [(M, 10), (N, 4), (D, 2), (M, 10), (N, 3), (I, 70), (M, 10)], flag=16),  # indels behind N do claim; 70 letters
        read(rng, 1299, [(H, 2), (S, 3), (M, 10), (I, 2), (EQ, 5), (D, 1), (X, 4), (N, 10), (P, 2), (M, 6), (S, 3), (H, 1)]),  # every op
        read(rng, 1399, [(M, 1)]), read(rng, 1400, [(M, 63)]), read(rng, 1401, [(M, 64)]), read(rng, 1460, [(M, 65)]),
        read(rng, 1500, [(M, 129)], flag=16), read(rng, 1520, [(M, 300)]),
        read(rng, 1530, [(M, 40)], seq="ACGTN" * 8),           # N in a read
        read(rng, 1840, [(D, 3)], seq="", qual=[]),            # empty seq: its indel's quality is 255
        read(rng, 1850, [(N, 5), (D, 2)], seq="", qual=[], flag=16),
        read(rng, 1950, [(M, 100)]),                           # ends behind the window
        read(rng, 499940, [(M, 30), (N, 30), (I, 2), (M, 20)], flag=16),  # an indel whose anchor is the last base of the step: lost
        read(rng, 499949, [(M, 100)]),                         # the step's last base inside a read
        read(rng, 499970, [(M, 10), (N, 5), (D, 2), (M, 30)]),
        read(rng, 499980, [(S, 4), (M, 10), (N, 30), (M, 10)]),
        read(rng, 500000, [(I, 3), (M, 40)]),                  # next step: un-anchored 500,001, anchor 500,000 before its window
        read(rng, 500010, [(M, 20), (D, 5), (M, 20)]),
        read(rng, 599990, [(M, 5), (N, 3), (D, 20), (M, 2)]),  # a deletion that runs past the contig's end
    ]
    r += [read(rng, 10, [(M, 30)], tid=2)]                     # ... and one behind it
    return r


def random_sample(rng, n_reads=26):
    """seeded reads over the windows: random CIGARs of every operation, lengths at and around the 64-lane stride"""
    starts = sorted(int(x) for x in np.concatenate([rng.integers(850, 2050, n_reads - 8), rng.integers(499880, 500070, 8)]))
    out = []
    for pos in starts:
        body = []
        for _ in range(int(rng.integers(1, 5))):
            body.append((int(rng.choice([M, M, EQ, X])), int(rng.choice([1, 7, 31, 63, 64, 65, 129]))))
            k = int(rng.integers(0, 7))
            if k < 4:
                body.append(([I, D, N, P][k], int(rng.integers(1, 6))))
        cigar = ([(H, 2)] if rng.random() < 0.1 else []) + ([(S, int(rng.integers(1, 9)))] if rng.random() < 0.3 else []) + body
        # the host advances the query on P as on S: a read with P needs that many bases to spare behind its last match
        pads = sum(ln for op, ln in body if op == P)
        cigar += [(S, 2 + pads)] if pads or rng.random() < 0.2 else []
        flag = (16 if rng.random() < 0.5 else 0) | (1024 if rng.random() < 0.05 else 0) | (512 if rng.random() < 0.05 else 0) | (4 if rng.random() < 0.03 else 0)
        rd = read(rng, pos, cigar, mapq=int(rng.choice([MAPQ_THD - 1, MAPQ_THD, 37, 60])), flag=flag)
        if rng.random() < 0.2:
            s = list(rd["seq"])
            s[int(rng.integers(0, len(s)))] = "N"
            rd["seq"] = "".join(s)
        out.append(rd)
    return out


class Corpus:
    """n BAM files (sample 0 the special one) and their FASTA under `directory`, written once"""

    def __init__(self, directory, n, seed=20):
        os.makedirs(str(directory), exist_ok=True)
        self.fa = reference()
        self.fasta = os.path.join(str(directory), "ref.fa")
        write_fasta(self.fasta, self.fa)
        self.bams, self.recs = [], []
        for s in range(n):
            rng = np.random.default_rng(seed + s)
            recs = special_sample(rng) if s == 0 else random_sample(rng)
            if s and s % 7 == 3:
                recs = []  # a sample without reads
            path = os.path.join(str(directory), "s%03d.bam" % s)
            bam_py.write_bam(path, REFS, recs, block_payload=700 if s < 3 else 60000)  # records that cross BGZF members
            self.bams.append(path)
            self.recs.append(recs)


# ------------------------------------------------------------------------------------------------------------------- the harness
class Dump:
    pass


def parse(path):
    b = open(path, "rb").read()
    assert b[:4] == b"PLUP"
    d = Dump()
    d.status, d.fail_sample, d.fail_run, d.fail_at = struct.unpack_from("<IIIQ", b, 4)
    d.rows, d.n_samples, d.pitch, d.n_tokens, d.n_covered, d.text_bytes, d.tid, d.n_runs, rec_bytes = struct.unpack_from("<IIQIIQiIQ", b, 24)
    o = 24 + struct.calcsize("<IIQIIQiIQ")
    if d.status == 0:
        cells = d.rows * d.pitch
        shape = (d.rows, d.pitch)
        d.cell = np.frombuffer(b, np.uint8, cells, o).reshape(shape); o += cells
        d.qual = np.frombuffer(b, np.uint8, cells, o).reshape(shape); o += cells
        d.mapq = np.frombuffer(b, np.uint8, cells, o).reshape(shape); o += cells
        d.rank = np.frombuffer(b, "<u2", cells, o).reshape(shape); o += 2 * cells
        d.depth = np.frombuffer(b, "<u4", d.rows, o); o += 4 * d.rows
        d.tokens = np.frombuffer(b, TOKEN_DTYPE, d.n_tokens, o); o += 24 * d.n_tokens
        d.text = np.frombuffer(b, np.uint8, d.text_bytes, o); o += d.text_bytes
    d.run_off = np.frombuffer(b, "<u8", d.n_runs + 1, o).copy(); o += 8 * (d.n_runs + 1)
    d.run_sample = np.frombuffer(b, "<u4", d.n_runs, o).copy(); o += 4 * d.n_runs
    d.records = np.frombuffer(b, np.uint8, rec_bytes, o).copy(); o += rec_bytes
    assert o == len(b)
    return d


def run_bam(exe, out, corpus, n, window, split=False, bams=None, fasta=None):
    """the harness over the first n samples of the corpus: (Dump, its standard output); raises if host and core differ"""
    beg, end = window
    cmd = [exe, "bam", str(out), fasta or corpus.fasta, REF_ID, str(REGION[0]), str(REGION[1]), str(beg), str(end), str(MAPQ_THD), "1" if split else "0"]
    p = subprocess.run(cmd + list(bams if bams is not None else corpus.bams[:n]), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("pileup_core_check: exit %d\n%s\n%s" % (p.returncode, p.stdout.decode(), p.stderr.decode()[-3000:]))
    return parse(out), p.stdout.decode()


def write_runs(path, runs, run_sample, n_samples):
    off = np.zeros(len(runs) + 1, "<u8")
    off[1:] = np.cumsum([len(r) for r in runs])
    with open(path, "wb") as f:
        f.write(struct.pack("<II", len(runs), n_samples) + off.tobytes() + np.asarray(run_sample, "<u4").tobytes() + b"".join(bytes(r) for r in runs))


def run_raw(exe, out, tmp, fa, runs, run_sample, n_samples, window, tid=TID, region=REGION, mapq_thd=MAPQ_THD):
    """the core alone over runs of bytes: (Dump, standard output); raises on a sanitizer report or any other non-zero exit"""
    ref_path, runs_path = os.path.join(str(tmp), "ref.bin"), os.path.join(str(tmp), "runs.bin")
    with open(ref_path, "wb") as f:
        f.write(fa.encode() if isinstance(fa, str) else bytes(fa))
    write_runs(runs_path, runs, run_sample, n_samples)
    p = subprocess.run([exe, "raw", str(out), ref_path, str(tid), str(region[0]), str(region[1]), str(window[0]), str(window[1]), str(mapq_thd), runs_path],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("pileup_core_check: exit %d\n%s\n%s" % (p.returncode, p.stdout.decode(), p.stderr.decode()[-3000:]))
    return parse(out), p.stdout.decode()


def record_bytes(r):
    """one record as BAM holds it (block_size word + block), as bam_py.write_bam packs it"""
    code = {c: i for i, c in enumerate(bam_py.BASES)}
    name = r.get("name", "r").encode() + b"\0"
    seq = r["seq"]
    packed = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= code[c] << (4 if i % 2 == 0 else 0)
    cig = b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in r["cigar"])
    body = struct.pack("<iiBBHHHiiii", r["tid"], r["pos"], len(name), r["mapq"], 4680, len(r["cigar"]), r["flag"], len(seq), -1, -1, 0) + name + cig + bytes(packed) + bytes(r["qual"])
    return struct.pack("<i", len(body)) + body


# --------------------------------------------------------------------------------------------- against the independent derivation
def step_of(window):
    gb = REGION[0] + (window[0] - REGION[0]) // STEP * STEP
    return gb, min(REGION[1], gb + STEP - 1)


def check_against_bam_py(d, recs_of, fa, window):
    """the dumped planes, depths and tokens against bam_py.pileup_sample, cell by cell"""
    beg, end = window
    gb, ge = step_of(window)
    tok = {(int(t["pos"]), int(t["sample"])): d.text[int(t["text_off"]):int(t["text_off"]) + int(t["text_len"])].tobytes().decode() for t in d.tokens}
    assert len(tok) == d.n_tokens
    depth = np.zeros(d.rows, np.int64)
    used = 0
    for s in range(d.n_samples):
        cells = bam_py.pileup_sample(recs_of[s], TID, fa, gb, ge, MAPQ_THD)
        for pos in range(beg, end + 1):
            row = pos - beg
            c, q, mq, rk = int(d.cell[row, s]), int(d.qual[row, s]), int(d.mapq[row, s]), int(d.rank[row, s])
            want = cells.get(pos)
            if want is None:
                assert (c, q, mq, rk) == (8, 0, 0, 0), (s, pos)
                continue
            depth[row] += 1
            if c & 8:
                base = "N" if (c & 3) == 0 else tok[(pos, s)]
                used += (c & 3) != 0
                assert (c & 3) == 0 or base[0] == "+-"[(c & 3) - 1]
            else:
                base = "ACGT"[c & 3]
            got = (mq, base, (q + 33) & 0xFF, rk, "-" if c & 4 else "+")
            assert got == (want[0], want[1], ord(want[2]) & 0xFF, min(want[3], 65535), want[4]), (s, pos, got, want)
    assert used == d.n_tokens
    assert (d.cell[:, d.n_samples:] == 8).all() and not d.rank[:, d.n_samples:].any()
    assert (depth == d.depth).all() and d.n_covered == int((depth > 0).sum())
