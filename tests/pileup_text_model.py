"""What the tests of bv_engine_pileup_text share.

`rows_text` is a serial restatement of the row format from its definition (the head of basevar_amd/csrc/bv_pileup_text_core.h):
Python string formatting, one row at a time; it shares no code with the core.  Beside it: the tile file that the stand-alone
harness tests/cpp/pileup_text_check.cpp reads, the harness's build and run, the parse of the reference's own rows
(tests/golden/reference_pileup_rows.txt.gz) back into planes and tokens, and the seeded tiles of the GPU tests."""
import gzip
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SRC = os.path.join(ROOT, "tests", "cpp", "pileup_text_check.cpp")
DEPS = [SRC, os.path.join(ROOT, "basevar_amd", "csrc", "bv_pileup_text_core.h"), os.path.join(ROOT, "basevar_amd", "host", "pileup.hpp"),
        os.path.join(ROOT, "basevar_amd", "host", "bamio.hpp"), os.path.join(ROOT, "basevar_amd", "host", "batchfile.hpp"),
        os.path.join(ROOT, "basevar_amd", "host", "bgzf_tabix.hpp"), os.path.join(ROOT, "include", "basevar_amd.h")]
OUT_DIR = os.path.join(ROOT, "basevar_amd", "lib", "san")
GOLDEN_ROWS = os.path.join(ROOT, "tests", "golden", "reference_pileup_rows.txt.gz")
TOKEN_DTYPE = np.dtype([("pos", "<u4"), ("sample", "<u4"), ("text_off", "<u8"), ("text_len", "<u4"), ("reserved_", "<u4")])
CELL_REV, CELL_N, CELL_INS, CELL_DEL = 0x04, 0x08, 0x09, 0x0A


class Tile:
    """planes [rows][pitch] (numpy), beg, n samples, tokens {(pos, sample): bytes}, the reference's bytes (ref[pos - 1]), CHROM"""

    def __init__(self, chrom, beg, n, cell, qual, mapq, rank, tokens, ref):
        self.chrom = chrom if isinstance(chrom, bytes) else chrom.encode()
        self.beg, self.n = int(beg), int(n)
        self.cell, self.qual, self.mapq = (np.ascontiguousarray(x, np.uint8) for x in (cell, qual, mapq))
        self.rank = np.ascontiguousarray(rank, np.uint16)
        self.rows, self.pitch = self.cell.shape
        self.tokens = dict(tokens)
        self.ref = ref if isinstance(ref, bytes) else ref.encode()

    def token_arrays(self):
        """(tokens sorted by (pos, sample) as TOKEN_DTYPE, their text back to back)"""
        keys = sorted(self.tokens)
        tok = np.zeros(len(keys), TOKEN_DTYPE)
        at = 0
        for i, k in enumerate(keys):
            tok[i] = (k[0], k[1], at, len(self.tokens[k]), 0)
            at += len(self.tokens[k])
        return tok, np.frombuffer(b"".join(self.tokens[k] for k in keys), np.uint8)


# ------------------------------------------------------------------------------------------------------------------- the model
def rows_text(t, first=0, n_rows=None):
    """(text, row_off) of rows [first, first + n_rows) of the tile, from the definition.  KeyError((pos, sample)) for an indel cell
    that has no token."""
    n_rows = t.rows - first if n_rows is None else n_rows
    out, off = [], [0]
    for r in range(first, first + n_rows):
        pos = t.beg + r
        m, b, q, k, s = [], [], [], [], []
        depth = 0
        for i in range(t.n):
            rank = int(t.rank[r, i])
            if rank == 0:
                m.append(b"0"); b.append(b"N"); q.append(b"!"); k.append(b"0"); s.append(b".")
                continue
            depth += 1
            c = int(t.cell[r, i])
            m.append(b"%d" % int(t.mapq[r, i]))
            if not c & 0x08:
                b.append(b"ACGT"[c & 3:(c & 3) + 1])
            elif c & 3 == 0:
                b.append(b"N")
            else:
                b.append(t.tokens[(pos, i)])
            q.append(bytes([(int(t.qual[r, i]) + 33) % 256]))
            k.append(b"%d" % rank)
            s.append(b"-" if c & 0x04 else b"+")
        row = b"\t".join([t.chrom, b"%d" % pos, t.ref[pos - 1:pos], b"%d" % depth] + [b" ".join(x) for x in (m, b, q, k, s)]) + b"\n"
        out.append(row)
        off.append(off[-1] + len(row))
    return b"".join(out), np.array(off, np.uint64)


def row_places(t, tile_samples, first=0, n_rows=None):
    """for the alignment census: per row of rows_text's text its start, the starts of its five lists, and inside each list the
    offsets at which the samples k * tile_samples begin (all offsets into the text of the asked-for rows)"""
    n_rows = t.rows - first if n_rows is None else n_rows
    out, at = [], 0
    for r in range(first, first + n_rows):
        pos = t.beg + r
        claimed = t.rank[r, :t.n] != 0
        head = len(t.chrom) + 1 + len(str(pos)) + 3 + len(str(int(claimed.sum()))) + 1
        lens = np.ones((5, t.n), np.int64)
        for i in np.nonzero(claimed)[0]:
            c = int(t.cell[r, i])
            lens[0, i] = len(str(int(t.mapq[r, i])))
            lens[3, i] = len(str(int(t.rank[r, i])))
            if c & 0x08 and c & 3:
                lens[1, i] = len(t.tokens[(pos, int(i))])
        starts, cuts, o = [], [], at + head
        for l in range(5):
            starts.append(o)
            before = np.concatenate([[0], np.cumsum(lens[l] + 1)])
            cuts.append([o + int(before[k]) for k in range(tile_samples, t.n, tile_samples)])
            o += int(before[-1])
        out.append((at, starts, cuts))
        at = o
    return out, at


# ------------------------------------------------------------------------------------------------------------------- the harness
def build(asan=True):
    """The harness: with ASan + UBSan (a program of its own: it needs no preloaded runtime), or plain for its timing mode."""
    exe = os.path.join(OUT_DIR, "pileup_text_check" + (".asan" if asan else ""))
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in DEPS):
        return exe
    os.makedirs(OUT_DIR, exist_ok=True)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-fno-omit-frame-pointer"] if asan else ["-O2"]
    tmp = exe + ".%d.tmp" % os.getpid()
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include")] + flags + [SRC, "-lz", "-o", tmp])
    os.replace(tmp, exe)
    return exe


def write_tile(path, t, first=0, n_rows=None):
    n_rows = t.rows - first if n_rows is None else n_rows
    tok, text = t.token_arrays()
    with open(path, "wb") as f:
        f.write(b"PTIL" + struct.pack("<8I2Q", t.beg, t.rows, t.n, t.pitch, len(tok), len(t.chrom), first, n_rows, len(text), len(t.ref)))
        f.write(t.chrom + t.ref + t.cell.tobytes() + t.qual.tobytes() + t.mapq.tobytes() + t.rank.tobytes() + tok.tobytes() + text.tobytes())


def run_tile(exe, tmp, t, first=0, n_rows=None):
    """the harness over one tile: (text, row_off) of the asked-for rows -- held to the host writer inside the harness --, or
    ("missing", pos, sample); raises on a sanitizer report, a difference or any other non-zero exit"""
    src, dst = os.path.join(str(tmp), "tile.bin"), os.path.join(str(tmp), "text.out")
    write_tile(src, t, first, n_rows)
    p = subprocess.run([exe, "tile", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("pileup_text_check: exit %d\n%s\n%s" % (p.returncode, p.stdout.decode(), p.stderr.decode()[-3000:]))
    b = open(dst, "rb").read()
    assert b[:4] == b"PTXT"
    status, n, bad_pos, bad_sample = struct.unpack_from("<4I", b, 4)
    if status:
        return "missing", bad_pos, bad_sample
    off = np.frombuffer(b, "<u8", n + 1, 20)
    text = b[20 + 8 * (n + 1):]
    assert len(text) == int(off[n])
    return text, off.copy()


# ------------------------------------------------------------------------------------------------------ the reference's own rows
def golden_rounds():
    """[(round, its bytes)] of tests/golden/reference_pileup_rows.txt.gz"""
    b = gzip.open(GOLDEN_ROWS, "rb").read()
    out, at = [], 0
    while at < len(b):
        nl = b.index(b"\n", at)
        word, r, size = b[at:nl].split()
        assert word == b"ROUND"
        out.append((int(r), b[nl + 1:nl + 1 + int(size)]))
        at = nl + 1 + int(size)
    return out


def parse_rows(text):
    """rows of batchfile text back into a Tile: a cell is unclaimed exactly where its strand token is '.'"""
    lines = text.split(b"\n")
    assert lines[-1] == b""
    lines = lines[:-1]
    first = lines[0].split(b"\t")
    chrom, beg, n = first[0], int(first[1]), len(first[8].split(b" "))
    pitch = (n + 15) // 16 * 16
    cell = np.full((len(lines), pitch), CELL_N, np.uint8)
    qual, mapq, rank = np.zeros_like(cell), np.zeros_like(cell), np.zeros(cell.shape, np.uint16)
    ref = bytearray(b"A" * (beg + len(lines) - 1))
    tokens = {}
    for r, line in enumerate(lines):
        f = line.split(b"\t")
        assert len(f) == 9 and f[0] == chrom and int(f[1]) == beg + r and len(f[2]) == 1
        ref[beg + r - 1] = f[2][0]
        m, b, q, k, s = (x.split(b" ") for x in f[4:])
        assert len(m) == len(b) == len(q) == len(k) == len(s) == n
        depth = 0
        for i in range(n):
            if s[i] == b".":
                assert (m[i], b[i], q[i], k[i]) == (b"0", b"N", b"!", b"0")
                continue
            depth += 1
            rev = CELL_REV if s[i] == b"-" else 0
            if b[i] in (b"A", b"C", b"G", b"T"):
                cell[r, i] = b"ACGT".index(b[i]) | rev
            elif b[i] == b"N":
                cell[r, i] = CELL_N | rev
            else:
                cell[r, i] = (CELL_INS if b[i][:1] == b"+" else CELL_DEL) | rev
                assert b[i][:1] in (b"+", b"-")
                tokens[(beg + r, i)] = b[i]
            mapq[r, i], qual[r, i], rank[r, i] = int(m[i]), (q[i][0] - 33) % 256, int(k[i])
            assert rank[r, i] != 0
        assert depth == int(f[3])
    return Tile(chrom, beg, n, cell, qual, mapq, rank, tokens, bytes(ref))


# ------------------------------------------------------------------------------------------------------------- seeded tiles
def random_tile(seed, n, rows, coverage, beg=1000, pitch_extra=0, chrom=b"chr7", long_tokens=(), indel_frac=0.08):
    """a seeded tile: claimed cells at `coverage`, every value over its whole range, random bytes in unclaimed cells' other planes
    and in the pitch's padding.  long_tokens: token lengths (bytes) dealt to the first indel cells."""
    rng = np.random.default_rng(seed)
    pitch = (n + 15) // 16 * 16 + pitch_extra
    shape = (rows, pitch)
    cell = rng.integers(0, 16, shape, dtype=np.uint8)
    qual = rng.integers(0, 256, shape, dtype=np.uint8)
    mapq = rng.integers(0, 256, shape, dtype=np.uint8)
    small = rng.integers(1, 151, shape)
    rank = np.where(rng.random(shape) < 0.15, rng.integers(1, 65536, shape), small).astype(np.uint16)
    claimed = rng.random(shape) < coverage if 0 < coverage < 1 else np.full(shape, coverage >= 1)
    claimed[:, n:] = rng.random((rows, pitch - n)) < 0.5  # the padding holds anything
    rank[~claimed] = 0
    # claimed cells of the samples: a base, N, or an indel with its token
    kind = rng.random(shape)
    base = rng.integers(0, 4, shape, dtype=np.uint8) | (rng.integers(0, 2, shape, dtype=np.uint8) << 2)
    rev = base & 4
    live = np.zeros(shape, bool)
    live[:, :n] = claimed[:, :n]
    cell = np.where(live, np.where(kind < indel_frac, np.where(kind < indel_frac / 2, CELL_INS, CELL_DEL) | rev, np.where(kind < indel_frac + 0.05, CELL_N | rev, base)), cell).astype(np.uint8)
    tokens = {}
    todo = list(long_tokens)
    for r, i in zip(*np.nonzero(live & ((cell & 0x0B) > 8))):
        ln = todo.pop(0) if todo else int(rng.integers(2, 7))
        body = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), ln - 1))
        tokens[(beg + int(r), int(i))] = (b"+" if cell[r, i] & 3 == 1 else b"-") + body
    ref = bytes(rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8), beg + rows + 3))
    t = Tile(chrom, beg, n, cell, qual, mapq, rank, tokens, ref)
    t.unused_long = len(todo)
    return t


def from_dump(d, chrom, fa, beg):
    """a pileup_ref Dump (planes, tokens and text of a pileup of the window that begins at `beg`) as a Tile"""
    tokens = {(int(k["pos"]), int(k["sample"])): d.text[int(k["text_off"]):int(k["text_off"]) + int(k["text_len"])].tobytes() for k in d.tokens}
    return Tile(chrom, beg, d.n_samples, d.cell, d.qual, d.mapq, d.rank, tokens, fa)
