"""What the tests of bv_engine_vcf_format share: the stand-alone harness tests/cpp/vcf_lines_check.cpp -- the host formatter's
lines (host/vcf_emit.hpp: format_vcf_line, the authority for the bytes), checked on the way against the serial builder of
basevar_amd/csrc/bv_vcf_core.h -- built with g++ and run as a program, and seeded records to feed it."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "vcf_lines_check.cpp")
DEPS = [SRC, os.path.join(ROOT, "basevar_amd", "csrc", "bv_vcf_core.h"), os.path.join(ROOT, "basevar_amd", "host", "vcf_emit.hpp"),
        os.path.join(ROOT, "basevar_amd", "host", "batchfile.hpp"), os.path.join(ROOT, "include", "basevar_amd.h")]
OUT_DIR = os.path.join(ROOT, "basevar_amd", "lib", "san")

BASES = b"ACGT"
CELL_VALUES = list(range(8)) + [0x08, 0x09, 0x0A]  # every value the planes hold: base | strand, BV_CELL_N, _INS, _DEL


def build(asan=False):
    """The harness: plain, or with ASan + UBSan (a program of its own: it needs no preloaded runtime)."""
    exe = os.path.join(OUT_DIR, "vcf_lines_check" + (".asan" if asan else ""))
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in DEPS):
        return exe
    os.makedirs(OUT_DIR, exist_ok=True)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g"] if asan else ["-O1"]
    tmp = exe + ".%d.tmp" % os.getpid()
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")] + flags + [SRC, "-o", tmp])
    os.replace(tmp, exe)
    return exe


def record(rng, alts, n_groups=0):
    """A seeded bv_site_result with the ALT bases `alts` (codes 0 .. 3, in order), and n_groups bv_group_result records"""
    from basevar_amd import _capi
    r = np.zeros((), dtype=_capi.SITE_DTYPE)
    r["depth"] = rng.integers(0, 5000, 4)
    r["total_depth"] = int(r["depth"].sum())
    r["status"] = 3
    r["cvg_sb"] = rng.integers(0, 3000, 4)
    r["cvg_fs"], r["cvg_sor"] = rng.random() * 30, rng.random() * 4
    r["n_alt"] = len(alts)
    r["alt"][:len(alts)] = alts
    r["af"][:len(alts)] = rng.random(len(alts)) * [1.0, 1e-3, 1e-7, 1.0][:len(alts)]
    r["caf"][:len(alts)] = rng.random(len(alts))
    r["qual"] = [rng.random() * 5000, rng.random() * 20, 20.0, 1e7 * rng.random()][int(rng.integers(0, 4))]
    r["qd"] = rng.random() * 40
    r["var_sb"] = rng.integers(0, 3000, 4)
    r["var_fs"], r["var_sor"] = rng.random() * 30, rng.random() * 4
    r["mq_ranksum"], r["rpr_ranksum"], r["bq_ranksum"] = rng.random(3) * 60 - 30
    g = np.zeros(n_groups, dtype=_capi.GROUP_DTYPE)
    for k in range(n_groups):
        na = int(rng.integers(0, len(alts) + 1))  # (a group without ALT prints nothing)
        g[k]["n_alt"] = na
        g[k]["alt"][:na] = alts[:na]
        g[k]["af"][:na] = rng.random(na)
        g[k]["total_depth"] = int(rng.integers(0, 1000))
    return r, g


def line(site, rec, groups=None, ref_base=b"A", ref_pos=1000, ref_id=b"chr1", head=None):
    return dict(site=int(site), rec=rec, groups=groups, ref_base=bytes(ref_base), ref_pos=int(ref_pos), ref_id=bytes(ref_id), head=head)


def run(exe, cell, phred, lines, group_names=(), tmp_dir="."):
    """[(head, gt uint8 [4], line)] for `lines` over the rows cell / phred [n_rows][n_samples]; raises if the harness finds the
    core header and the host formatter apart."""
    cell = np.ascontiguousarray(cell, dtype=np.uint8)
    phred = np.ascontiguousarray(phred, dtype=np.uint8)
    n_rows, n = cell.shape
    assert phred.shape == cell.shape
    parts = [struct.pack("<4I", n_rows, n, len(lines), len(group_names))]
    for g in group_names:
        parts += [struct.pack("<I", len(g)), bytes(g)]
    parts += [cell.tobytes(), phred.tobytes()]
    for ln in lines:
        parts += [struct.pack("<III", ln["site"], ln["ref_pos"], len(ln["ref_id"])), ln["ref_id"], struct.pack("<I", len(ln["ref_base"])), ln["ref_base"]]
        parts += [struct.pack("<i", -1)] if ln["head"] is None else [struct.pack("<i", len(ln["head"])), bytes(ln["head"])]
        parts.append(ln["rec"].tobytes())
        if group_names:
            assert ln["groups"] is not None and len(ln["groups"]) == len(group_names)
            parts.append(ln["groups"].tobytes())
    fin, fout = os.path.join(str(tmp_dir), "vcf_lines.in"), os.path.join(str(tmp_dir), "vcf_lines.out")
    with open(fin, "wb") as f:
        f.write(b"".join(parts))
    p = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("vcf_lines_check exit %d: %s" % (p.returncode, p.stderr.decode(errors="replace")))
    data = open(fout, "rb").read()
    out, at = [], 0
    for _ in lines:
        (hl,) = struct.unpack_from("<I", data, at)
        head = data[at + 4:at + 4 + hl]
        at += 4 + hl
        gt = np.frombuffer(data[at:at + 4], dtype=np.uint8).copy()
        (ll,) = struct.unpack_from("<Q", data, at + 4)
        out.append((head, gt, data[at + 12:at + 12 + ll]))
        at += 12 + ll
    assert at == len(data)
    return out


def py_line(head, gt, cell, phred):
    """the definition at the head of bv_vcf_core.h, written out once more in Python (a cross-check of the harness's plumbing)"""
    import math
    toks = []
    for c, q in zip(cell.tolist(), phred.tolist()):
        if c & 8:
            toks.append(b"./.")
            continue
        g = bytes([gt[c & 3]])
        toks.append((b"0/." if g == b"0" else b"./" + g) + b":" + BASES[c & 3:(c & 3) + 1] + b":" + (b"-" if c & 4 else b"+") + b":" +
                    ("%f" % (1.0 - math.exp(q * -0.23025850929940458))).encode())
    return bytes(head) + b"".join(b"\t" + t for t in toks) + b"\n"
