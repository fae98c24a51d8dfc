"""What the tests of the device's indel tally share (include/basevar_amd_indel.h): the stand-alone harness
tests/cpp/indel_tally_check.cpp -- basevar_amd/csrc/bv_indel_tally_core.h held to host/vcf_emit.hpp's indel_string, the authority
for the bytes -- built with g++ and run as a program; a serial model that shares no code with either; and the corpus of rows."""
import collections
import os
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "indel_tally_check.cpp")
CORE = os.path.join(ROOT, "basevar_amd", "csrc", "bv_indel_tally_core.h")
DEPS = [SRC, CORE] + [os.path.join(ROOT, *p) for p in (("basevar_amd", "host", "vcf_emit.hpp"), ("basevar_amd", "host", "batchfile.hpp"), ("include", "basevar_amd.h"))]
OUT_DIR = os.path.join(ROOT, "basevar_amd", "lib", "san")
TOKEN_DTYPE = np.dtype([("pos", "<u4"), ("sample", "<u4"), ("text_off", "<u8"), ("text_len", "<u4"), ("reserved_", "<u4")])  # bv_pileup_token
COLUMN_MAX = 16384
LIMIT = int(re.search(r"#define BV_INDEL_ROW_TOKENS_MAX (\d+)u", open(CORE).read()).group(1))


def build(asan=False):
    """The harness: plain, or with ASan + UBSan (a program of its own: it needs no preloaded runtime)."""
    exe = os.path.join(OUT_DIR, "indel_tally_check" + (".asan" if asan else ""))
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in DEPS):
        return exe
    os.makedirs(OUT_DIR, exist_ok=True)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g"] if asan else ["-O2"]
    tmp = exe + ".%d.tmp" % os.getpid()
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")] + flags + [SRC, "-o", tmp])
    os.replace(tmp, exe)
    return exe


def model_column(tokens):
    """The row's column, b"" for ".": sorted(Counter) on bytes -- Python orders bytes as unsigned, a proper prefix first"""
    tally = collections.Counter(t for t in tokens if t and t[:1] not in (b"N", b"A", b"C", b"G", b"T"))
    return b",".join(t + b"|%d" % tally[t] for t in sorted(tally))


def model_row(tokens):
    """(flag, column) as bv_engine_indel_tally defines them"""
    col = model_column(tokens)
    return (1, b"") if len(tokens) > LIMIT or len(col) > COLUMN_MAX else (0, col)


class Rows:
    """Rows as (pos, [token, ...]) in the order given -> tokens ascending by pos over one text, and the keys asked for.  The text
    begins with `lead` bytes no token uses, so that the whole layout can be shifted."""
    def __init__(self, rows, keys, lead=0):
        self.rows = collections.OrderedDict()
        for pos, toks in rows:
            assert pos not in self.rows
            self.rows[pos] = [bytes(t) for t in toks]
        self.keys = np.array(keys, dtype=np.uint32)
        n = sum(len(t) for t in self.rows.values())
        self.tokens = np.zeros(n, dtype=TOKEN_DTYPE)
        parts, at, i = [b"\xee" * lead], lead, 0
        for pos in sorted(self.rows):
            for s, t in enumerate(self.rows[pos]):
                self.tokens[i] = (pos, s, at, len(t), 0)
                parts.append(t)
                at += len(t)
                i += 1
        self.text = np.frombuffer(b"".join(parts) or b"", dtype=np.uint8).copy()

    @classmethod
    def from_arrays(cls, tokens, text, keys):
        """Rows over tokens and text as an engine handed them out (bv_pileup_token records sorted by pos)"""
        self = cls([], keys)
        self.tokens, self.text = np.ascontiguousarray(tokens, dtype=TOKEN_DTYPE), np.ascontiguousarray(text, dtype=np.uint8)
        raw = self.text.tobytes()
        for t in self.tokens:
            self.rows.setdefault(int(t["pos"]), []).append(raw[int(t["text_off"]):int(t["text_off"]) + int(t["text_len"])])
        return self

    def tokens_of(self, key):
        return self.rows.get(int(key), [])

    def expected(self):
        """[(flag, column)] per key, by the model"""
        return [model_row(self.tokens_of(k)) for k in self.keys]


def write_input(path, rows):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQI", len(rows.tokens), len(rows.text), len(rows.keys)) + rows.tokens.tobytes() + rows.text.tobytes() + rows.keys.tobytes())


def run_rows(exe, rows, tmp_dir="."):
    """[(flag, tokens of the row, classes, greatest count, column)] per key from the harness, which exits non-zero where the
    core and indel_string part"""
    fin, fout = os.path.join(str(tmp_dir), "indel_tally.in"), os.path.join(str(tmp_dir), "indel_tally.out")
    write_input(fin, rows)
    p = subprocess.run([exe, "rows", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("indel_tally_check rows exit %d: %s" % (p.returncode, p.stderr.decode(errors="replace")[-2000:]))
    data, out, at = open(fout, "rb").read(), [], 0
    for _ in rows.keys:
        flag, n, classes, most, size = struct.unpack_from("<BIIII", data, at)
        at += 17
        out.append((flag, n, classes, most, data[at:at + size]))
        at += size
    assert at == len(data)
    return out


def run_order(exe):
    p = subprocess.run([exe, "order"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("indel_tally_check order exit %d: %s" % (p.returncode, p.stderr.decode(errors="replace")[-2000:]))
    return int(re.search(r"order: (\d+) pairs", p.stdout.decode()).group(1))


def distinct(i, width=0):
    """the i-th of a family of distinct tokens: '+' and i in base 4 as letters, at least `width` of them"""
    s = b""
    while i or len(s) < max(1, width):
        s = b"ACGT"[i % 4:i % 4 + 1] + s
        i //= 4
    return b"+" + s


def cycle(classes, n):
    return [classes[i % len(classes)] for i in range(n)]


def corpus(lead=0):
    """The rows every test of the tally runs: see tests/test_indel_tally_cpu.py, which asserts from the harness's dump that
    each case is reached.  Returns Rows; rows are named in .names (name -> pos)."""
    rng = np.random.default_rng(20240917)
    rows, names = [], {}
    pos = [1000]

    def add(name, toks, gap=1):
        pos[0] += gap
        rows.append((pos[0], toks))
        names[name] = pos[0]

    # ---- order
    add("plus_minus", [b"-AT", b"+AT", b"-AT"])
    add("prefix", [b"+AC", b"+A", b"+ACG", b"+A"])
    add("high_byte_in_key", [b"+A\x80", b"+Aa", b"+A\xff", b"+A\x7f"])           # the deciding byte inside the 4-byte key
    add("high_byte_beyond_key", [b"+ACGT\x80T", b"+ACGTaT", b"+ACGT\xffT", b"+ACGT"])  # ... and behind it
    P = bytes(b"ACGT"[(7 * i) % 4] for i in range(80))
    for k in (15, 16, 17, 63, 64, 65):  # texts equal up to their k-th byte, which decides; and the proper prefix of k - 1 bytes
        add("equal_to_%d" % k, [b"+" + P[:k - 2] + b"t", b"+" + P[:k - 2] + b"g", b"+" + P[:k - 2], b"+" + P[:k - 2] + b"g"])
    add("one_byte", [b"+", b"+A", b"+", b"-"])
    X = b"-" + bytes(b"ACGT"[(5 * i + i // 7) % 4] for i in range(8999))
    add("long_equal", [X, X])
    add("long_last_byte", [X[:-1] + b"a", X[:-1] + b"c"])  # two classes of 9,000 bytes: beyond the column's bound, so flagged
    # ---- row sizes
    three = [b"+AT", b"-C", b"+ATT"]
    for n in (1, 2, 63, 64, 65, 127, 128, 129):
        add("size_%d" % n, cycle(three, n))
    eight = [distinct(i, 2) for i in range(8)]
    for n in (LIMIT - 1, LIMIT, LIMIT + 1):
        add("size_%d" % n, cycle(eight, n))
    # ---- classes
    for c in (1, 2, 63, 64, 65):
        add("classes_%d" % c, cycle([distinct(i, 3) for i in range(c)], 2 * c + 1))
    for n in (64, 65, 300):
        add("all_distinct_%d" % n, [distinct(int(i)) for i in rng.permutation(n)])
    # ---- counts
    toks = sum(([distinct(j, 4)] * c for j, c in enumerate((1, 9, 10, 99, 100, 9999))), [])
    add("counts", [toks[int(i)] for i in rng.permutation(len(toks))])
    add("count_10000", [b"-G"] * 10000)
    # ---- column length
    add("column_16384_one", [b"+" + b"A" * (COLUMN_MAX - 3)])   # text '|' '1'
    add("column_16385_one", [b"+" + b"A" * (COLUMN_MAX - 2)])
    many =[bytes([a, b]) for a in range(97, 123) for b in range(33, 160)][:3277]         # "xy|1,": 5 x 3277 - 1 = 16,384
    add("column_16384_many", many)
    add("column_16385_many", many + [many[5]] * 9)                                        # one count of 10: a byte more
    # ---- the filter, as a host caller may hand tokens in
    add("filter", [b"", b"N", b"A+", b"+A", b"C", b"G", b"T", b"-C", b"", b"+A", b"NN"])
    add("filter_all", [b"", b"A", b"N"])
    # ---- keys: rows without tokens between rows with tokens, the same row shuffled, tokens no key asks for
    base = [b"+AT"] * 5 + [b"-CC"] * 3 + [b"+A", b"-C\x00", b"\x00+"]
    add("shuffle_a", base, gap=3)
    add("shuffle_b", [base[int(i)] for i in rng.permutation(len(base))], gap=2)
    add("unasked", [b"+TTTT"] * 7, gap=2)
    # ---- seeded rows over the whole byte range
    for r in range(24):
        classes = [bytes(rng.integers(0, 256, int(rng.integers(0, 21))).astype(np.uint8)) for _ in range(int(rng.integers(1, 12)))]
        classes.append(b"+" + bytes(range(11 * r, min(256, 11 * r + 11))))  # (every byte value, whatever the seed)
        add("seeded_%d" % r, [classes[int(i)] for i in rng.integers(0, len(classes), int(rng.integers(1, 200)))] + classes[-1:], gap=1 + r % 3)
    asked = [p for name, p in names.items() if name != "unasked"]
    first, last = min(asked), max(asked)
    between = [p for p in range(first, last) if p not in names.values()]
    # every row once in position order with the empty positions between them; then keys that match nothing, repeats, and all
    # of it again in reverse
    keys = sorted(asked + between) + [5, last + 10, 0xffffffff] + [names["plus_minus"], names["counts"], names["plus_minus"]]
    keys = keys + keys[::-1][:40]
    out = Rows(rows, keys, lead)
    out.names = names
    return out


def lines_tokens(lines):
    """The tokens of record_text_ref lines as Rows keyed by the line's index"""
    return Rows([(k, ln["tokens"]) for k, ln in enumerate(lines) if ln["tokens"]], list(range(len(lines))))
