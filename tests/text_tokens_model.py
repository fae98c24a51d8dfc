"""What the tests of the device's text tokens share (include/basevar_amd_text_tokens.h): a serial model of the definition at the
head of basevar_amd/csrc/bv_text_tokens_core.h that shares no code with it; the corpus of batches; and the stand-alone harness
tests/cpp/text_tokens_check.cpp -- the core held to the host reader (parse_site_rows_fast) and to BaseTypeEngine::finish_text's
walk -- built with g++ and run as a program."""
import gzip
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "text_tokens_check.cpp")
CORE = os.path.join(ROOT, "basevar_amd", "csrc", "bv_text_tokens_core.h")
DEPS = [SRC, CORE] + [os.path.join(ROOT, "basevar_amd", "host", h) for h in ("batchfile_fast.hpp", "basetype_gpu.hpp", "batchfile.hpp", "vcf_emit.hpp", "indel_tokens.hpp")]
OUT_DIR = os.path.join(ROOT, "basevar_amd", "lib", "san")
GOLDEN_ROWS = os.path.join(ROOT, "tests", "golden", "reference_pileup_rows.txt.gz")
SKIP, HOST, INDEL = 1, 2, 4  # BV_TEXT_*


# ------------------------------------------------------------------------------------------------------------------ the model
def model_tokens(rows, file_samples, state):
    """[(pos, sample, text)] of a batch: rows[p][f] bytes without the line break, state[p] the position's final state"""
    foff = np.concatenate([[0], np.cumsum(file_samples)[:-1]]).astype(int)
    out = []
    for p, files in enumerate(rows):
        if state[p]:
            continue
        for f, row in enumerate(files):
            for i, tok in enumerate(row.split(b"\t")[5].split(b" ")):
                if tok[:1] in (b"+", b"-"):
                    out.append((p, int(foff[f]) + i, tok))
    return out


def token_places(row):
    """[(offset of the token's first byte in the row, offset of the separator that ends it)] of the row's tokens, from its bytes"""
    f = row.split(b"\t")
    at, out = sum(len(x) + 1 for x in f[:5]), []
    for tok in f[5].split(b" "):
        if tok[:1] in (b"+", b"-"):
            out.append((at, at + len(tok)))
        at += len(tok) + 1
    return out


def marked(row):
    """the row holds a token: what BV_TEXT_INDEL says of a row the device parsed"""
    f = row.split(b"\t")
    return len(f) == 9 and any(t[:1] in (b"+", b"-") for t in f[5].split(b" "))


def tokens_of_arrays(tok, text):
    """[(pos, sample, text)] of descriptors and their text as an engine handed them out; the layout's promises are asserted"""
    raw = bytes(np.ascontiguousarray(text, np.uint8))
    out, end = [], 0
    for t in tok:
        off, n = int(t["text_off"]), int(t["text_len"])
        assert off >= end and n >= 1 and off + n <= len(raw) and int(t["reserved_"]) == 0, (off, n, end, len(raw))
        end = off + n
        out.append((int(t["pos"]), int(t["sample"]), raw[off:off + n]))
    return out


# ----------------------------------------------------------------------------------------------------------------- the corpus
def call(base=b"A", strand=b"+", qual=b"I", mapq=b"60", rank=b"9"):
    return (mapq, base, qual, rank, strand)


NOCALL = (b"0", b"N", b"!", b"0", b".")


def ind(text, strand=b"+"):
    return (b"37", text, b"5", b"12", strand)


def mkrow(chrom, pos, ref, samples, depth=None):
    """one batchfile row, without the line break"""
    if depth is None:
        depth = sum(1 for s in samples if s[4] != b".")
    cols = [b" ".join(s[c] for s in samples) for c in range(5)]
    return b"\t".join([chrom, b"%d" % pos, ref, b"%d" % depth] + cols)


def letters(n, salt=0):
    return bytes(b"ACGT"[(5 * i + i // 7 + salt) % 4] for i in range(n))


def golden_rounds():
    b = gzip.open(GOLDEN_ROWS, "rb").read()
    out, at = [], 0
    while at < len(b):
        nl = b.index(b"\n", at)
        word, r, size = b[at:nl].split()
        assert word == b"ROUND"
        out.append(b[nl + 1:nl + 1 + int(size)])
        at = nl + 1 + int(size)
    return out


class Batch:
    def __init__(self, name, rows, file_samples, state=None, chunk_bytes=0, host_skips=()):
        self.name, self.rows, self.file_samples = name, rows, list(file_samples)
        self.state = list(state) if state is not None else [0] * len(rows)  # the positions' final states, by construction
        self.chunk_bytes = chunk_bytes      # BASEVAR_AMD_TEXT_CHUNK_BYTES for bv_engine_text_parse (0: the default)
        self.host_skips = set(host_skips)   # positions the host reader is handed and skips
        assert all(len(r) == len(self.file_samples) for r in rows) and len(self.state) == len(rows)

    P = property(lambda self: len(self.rows))
    F = property(lambda self: len(self.file_samples))
    N = property(lambda self: sum(self.file_samples))

    def tokens(self):
        return model_tokens(self.rows, self.file_samples, self.state)

    def parse_state(self):
        """the positions' states as the parse reports them: a position the host reader skips is BV_TEXT_HOST until then"""
        return [HOST if p in self.host_skips else s for p, s in enumerate(self.state)]

    def chunks(self, cap_before=0):
        """[(first position, behind the last)] of the chunks bv_engine_text_parse cuts the batch into (whole positions, at most
        the stage's capacity) on an engine whose stage holds `cap_before` bytes already: the stage only grows, so a batch cut
        into several chunks on a fresh engine is ONE chunk on an engine that has parsed a larger batch before"""
        up = lambda x: (x + 255) // 256 * 256  # noqa: E731
        size = [sum(len(r) + 1 for r in files) for files in self.rows]
        cap = max(cap_before, up(max(size)), min(self.chunk_bytes or (128 << 20), up(sum(size))))
        out, p0 = [], 0
        while p0 < self.P:
            p1 = p0 + 1
            while p1 < self.P and sum(size[p0:p1 + 1]) <= cap:
                p1 += 1
            out.append((p0, p1))
            p0 = p1
        return out

    def packed(self):
        """(text uint8, row_off uint64): the rows back to back, each with its line break"""
        flat = [r + b"\n" for files in self.rows for r in files]
        off = np.zeros(len(flat) + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in flat])
        return np.frombuffer(b"".join(flat), np.uint8), off


def corpus():
    """The batches every test of the text tokens runs; tests/test_text_tokens_cpu.py asserts from the harness's dump that they
    reach the cases they are here for."""
    out = []
    A, N = call(), NOCALL
    # ---- one file, one sample, one position: the only token of its column
    out.append(Batch("only", [[mkrow(b"chr1", 7, b"A", [ind(b"+ACG")])]], [1]))
    # ---- a token's first byte (and every other byte of the column) on each lane: CHROM of 1 .. 65 bytes; 2 + 1 samples
    out.append(Batch("lanes", [[mkrow(b"c" * k, 100 + k, b"G", [A, ind(b"+AC")]), mkrow(b"c" * k, 100 + k, b"G", [ind(b"-G", b"-")])] for k in range(1, 66)], [2, 1]))
    # ---- lengths and places: 63 + 65 + 200 samples, two positions
    f0 = [N] * 63
    for at, t in ((0, b"+"), (2, b"-"), (5, b"+A"), (9, b"-" + letters(62)), (10, b"+" + letters(63, 1)), (20, b"-" + letters(64, 2)), (40, b"+" + letters(128, 3)), (61, A)):
        f0[at] = ind(t) if isinstance(t, bytes) else t
    f1 = [ind((b"+A", b"-C", b"+ACGT")[i % 3], b"+-"[i % 2:i % 2 + 1]) for i in range(65)]  # every sample a token
    f2 = [(ind(b"+A"), N, ind(b"-C"), N)[i % 4] for i in range(200)]
    g0 = [ind(b"-TT")] + [A] * 61 + [ind(b"+GGG")]                      # the first and the last token of the column (ended by the tab)
    g1 = [A] * 30 + [ind(b"+" + letters(8999)), ind(b"-" + letters(8999, 1))] + [N] * 33  # two long tokens back to back
    g2 = [A if i % 3 == 0 else N for i in range(200)]                  # an unmarked row behind marked ones
    out.append(Batch("lengths", [[mkrow(b"chr2", 500, b"C", f0), mkrow(b"chr2", 500, b"C", f1), mkrow(b"chr2", 500, b"C", f2)],
                                 [mkrow(b"chr2", 501, b"T", g0), mkrow(b"chr2", 501, b"T", g1), mkrow(b"chr2", 501, b"T", g2)]], [63, 65, 200]))
    # ---- 2 + 64 samples
    h1 = [ind(b"+" + letters(1 + i % 5, i)) if i % 9 == 4 else (A if i % 2 else N) for i in range(64)]
    out.append(Batch("two_files", [[mkrow(b"chrX", 9, b"a", [A, ind(b"-A")]), mkrow(b"chrX", 9, b"a", h1)],
                                   [mkrow(b"chrX", 10, b"c", [N, call(b"T", b"-")]), mkrow(b"chrX", 10, b"c", h1[::-1])]], [2, 64]))
    # ---- what must not be taken: a CHROM with '-' and '+', strands, qualities '+' (phred 10) and '-' (phred 12)
    q = [call(b"C", b"+", b"+"), call(b"G", b"-", b"-"), ind(b"+T", b"-")]
    out.append(Batch("not_taken", [[mkrow(b"HLA-A+1", 3, b"-", q), mkrow(b"HLA-A+1", 3, b"-", [call(b"T", b"-", b"-"), call(b"A", b"+", b"+")])],
                                   [mkrow(b"HLA-A+1", 2, b"+", q[:2] + [A]), mkrow(b"HLA-A+1", 2, b"+", [call(b"T", b"-", b"+"), call(b"A", b"+", b"-")])]], [3, 2]))
    # ---- no token at all
    out.append(Batch("none", [[mkrow(b"chr-3", 40 + p, b"G", q[:2]), mkrow(b"chr-3", 40 + p, b"G", [A, N, call(b"T", b"-", b"+")])] for p in range(3)], [2, 3]))
    # ---- positions that end BV_TEXT_SKIP or BV_TEXT_HOST, marked rows before and after each
    fs = [2, 3, 2]

    def ok(p, chrom=b"chr4"):
        return [mkrow(chrom, p, b"A", [A, ind(b"+A%d" % p)]), mkrow(chrom, p, b"A", [N, ind(b"-CC", b"-"), A]), mkrow(chrom, p, b"A", [ind(b"+"), N])]

    rows, state = [], []
    for p in range(11):
        r, s = ok(900 - p), 0  # (POS descends: pos is the position's index in the batch)
        if p == 1:   # Depth fields sum to 0 while the rows hold tokens
            r, s = [mkrow(b"chr4", 899, b"A", [A, ind(b"+SKIP")], 0), mkrow(b"chr4", 899, b"A", [N, ind(b"-SK"), A], 0), mkrow(b"chr4", 899, b"A", [N, N], 0)], SKIP
        elif p == 3:  # a defect in file 2's row behind file 0's marked row
            r[2], s = mkrow(b"chr4", 897, b"A", [call(b"AC"), ind(b"+HOST")]), HOST
        elif p == 5:  # a covered call with strand '.'
            r[1], s = mkrow(b"chr4", 895, b"A", [call(b"G", b"."), ind(b"-HO"), A]), HOST
        elif p == 7:  # a prefix of more than 512 bytes
            r, s = ok(893, b"chr4" + b"L" * 600), HOST
        elif p == 9:  # a position the host reader is handed and skips
            r, s = ok(891, b"skipme"), SKIP
            r[0] = mkrow(b"skipme", 891, b"A", [call(b"AC"), ind(b"+GONE")])
        rows.append(r)
        state.append(s)
    out.append(Batch("states", rows, fs, state, host_skips=[9]))
    # ---- three chunks and more on an engine that has staged nothing larger (Batch.chunks), every row marked: marked rows in
    # each chunk and as its first and last row; tokens of 70 bytes and more in every chunk, so that a token spans steps where
    # the chunk's text does not begin at the text's first byte, and the store is moved while it holds the chunks before
    out.append(Batch("chunks", [[mkrow(b"chr5", 70 + p, b"T", [A, ind(b"+C%d" % p), N]), mkrow(b"chr5", 70 + p, b"T", [ind(b"-" + letters(70 + 9 * p, p)), A, ind(b"+T")])]
                                for p in range(9)], [3, 3], chunk_bytes=512))
    # ---- the reference's own stored rows
    for k in (0, 5, 35):
        lines = golden_rounds()[k].split(b"\n")[:-1]
        out.append(Batch("golden_%d" % k, [[ln] for ln in lines], [len(lines[0].split(b"\t")[8].split(b" "))],
                         [0 if int(ln.split(b"\t")[3]) else SKIP for ln in lines]))  # (a Depth of 0 is a skipped position)
    return out


def host_reader(lines):
    """A lenient host reader for the positions left to the host: (cell, phred, mapq, rank, ref_code) rows, or None (skipped)
    for the positions whose CHROM says so"""
    if lines[0].startswith(b"skipme"):
        return None
    cell, phred, mapq, rank = [], [], [], []
    for ln in lines:
        f = ln.split(b"\t")
        for m, b, q, k, s in zip(*(x.split(b" ") for x in f[4:9])):
            c = {b"A": 0, b"C": 1, b"G": 2, b"T": 3}.get(b, 9 if b[:1] == b"+" else 10 if b[:1] == b"-" else 8)
            cell.append(c | 4 if c < 4 and s == b"-" else c)
            phred.append(q[0] - 33)
            mapq.append(int(m))
            rank.append(int(k))
    ref = lines[0].split(b"\t")[2][:1].upper()
    return (np.array(cell, np.uint8), np.array(phred, np.uint8), np.array(mapq, np.uint8), np.array(rank, np.uint16), b"ACGT".find(ref) if ref in b"ACGT" and ref else 4)


# ---------------------------------------------------------------------------------------------------------------- the harness
def build(asan=False):
    """The harness: plain, or with ASan + UBSan (a program of its own: it needs no preloaded runtime)."""
    exe = os.path.join(OUT_DIR, "text_tokens_check" + (".asan" if asan else ""))
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in DEPS):
        return exe
    os.makedirs(OUT_DIR, exist_ok=True)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g"] if asan else ["-O2"]
    tmp = exe + ".%d.tmp" % os.getpid()
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")] + flags + [SRC, "-o", tmp])
    os.replace(tmp, exe)
    return exe


def write_input(path, batches):
    with open(path, "wb") as f:
        f.write(struct.pack("<4sI", b"TTIN", len(batches)))
        for b in batches:
            f.write(struct.pack("<II", b.P, b.F) + np.asarray(b.file_samples, "<u4").tobytes() + bytes(b.state))
            for files in b.rows:
                for r in files:
                    f.write(struct.pack("<I", len(r) + 1) + r + b"\n")


def run(exe, batches, tmp_dir="."):
    """Per batch [(pos, sample, file, text)] as the core lists them; the harness has exited non-zero where the core, the host
    reader and finish_text's walk part."""
    fin, fout = os.path.join(str(tmp_dir), "text_tokens.in"), os.path.join(str(tmp_dir), "text_tokens.out")
    write_input(fin, batches)
    p = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("text_tokens_check exit %d: %s" % (p.returncode, p.stderr.decode(errors="replace")[-3000:]))
    data, at, out = open(fout, "rb").read(), 0, []
    for _ in batches:
        (n,) = struct.unpack_from("<Q", data, at)
        at += 8
        toks = []
        for _ in range(n):
            pos, sample, f, size = struct.unpack_from("<4I", data, at)
            at += 16
            toks.append((pos, sample, f, data[at:at + size]))
            at += size
        out.append(toks)
    assert at == len(data)
    return out
