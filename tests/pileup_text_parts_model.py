"""What the tests of bv_engine_pileup_text_parts share.

The rows of a sample part are DEFINED as the rows of a tile that holds only the part's columns ("ROWS OF A PART",
basevar_amd/csrc/bv_pileup_text_core.h).  `parts_text` is that sentence and nothing more: it slices the planes to the part's columns,
rebases the samples of the indel tokens and hands the slice to pileup_text_model.rows_text, the serial restatement of the row
format.  Beside it: the build and run of the stand-alone harness tests/cpp/pileup_text_parts_check.cpp."""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pileup_text_model as ptm  # noqa: E402

SRC = os.path.join(ROOT, "tests", "cpp", "pileup_text_parts_check.cpp")
DEPS = [SRC] + ptm.DEPS[1:]


def slice_tile(t, s0, s1):
    """the tile that holds only columns [s0, s1) of t; tokens of other columns are dropped, the others' samples rebased"""
    tokens = {(pos, s - s0): v for (pos, s), v in t.tokens.items() if s0 <= s < s1}
    return ptm.Tile(t.chrom, t.beg, s1 - s0, t.cell[:, s0:s1], t.qual[:, s0:s1], t.mapq[:, s0:s1], t.rank[:, s0:s1], tokens, t.ref)


def parts_text(t, part_first, first=0, n_rows=None):
    """(text, row_off) of rows [first, first + n_rows) of the parts, part-major: row k of part p is row_off[p * n_rows + k].
    KeyError((pos, absolute sample)) for an indel cell inside a part that has no token."""
    out, off = [], [np.zeros(1, np.uint64)]
    at = 0
    for p in range(len(part_first) - 1):
        s0, s1 = int(part_first[p]), int(part_first[p + 1])
        try:
            text, o = ptm.rows_text(slice_tile(t, s0, s1), first, n_rows)
        except KeyError as e:
            pos, s = e.args[0]
            raise KeyError((pos, s + s0))
        out.append(text)
        off.append(o[1:] + np.uint64(at))
        at += len(text)
    return b"".join(out), np.concatenate(off)


def part_starts(row_off, n_parts):
    """the offsets at which the parts' texts begin and the last one ends: block tables are cut there"""
    n = (len(row_off) - 1) // n_parts
    return [int(row_off[p * n]) for p in range(n_parts + 1)]


def build(asan=True):
    exe = os.path.join(ptm.OUT_DIR, "pileup_text_parts_check" + (".asan" if asan else ""))
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in DEPS):
        return exe
    os.makedirs(ptm.OUT_DIR, exist_ok=True)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-fno-omit-frame-pointer"] if asan else ["-O2"]
    tmp = exe + ".%d.tmp" % os.getpid()
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include")] + flags + [SRC, "-lz", "-o", tmp])
    os.replace(tmp, exe)
    return exe


def run_parts(exe, tmp, t, part_first, first=0, n_rows=None):
    """the harness over one tile and part table: (text, row_off) of the asked-for rows, part-major -- each part held to the host
    writer on the sliced tile inside the harness --, or ("missing", pos, absolute sample)"""
    src, dst = os.path.join(str(tmp), "tile.bin"), os.path.join(str(tmp), "parts.out")
    ptm.write_tile(src, t, first, n_rows)
    p = subprocess.run([exe, "tile", src, dst] + [str(int(x)) for x in part_first], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("pileup_text_parts_check: exit %d\n%s\n%s" % (p.returncode, p.stdout.decode(), p.stderr.decode()[-3000:]))
    b = open(dst, "rb").read()
    assert b[:4] == b"PTXT"
    status, n, bad_pos, bad_sample = struct.unpack_from("<4I", b, 4)
    if status:
        return "missing", bad_pos, bad_sample
    off = np.frombuffer(b, "<u8", n + 1, 20)
    text = b[20 + 8 * (n + 1):]
    assert len(text) == int(off[n])
    return text, off.copy()
