"""What the tests of the device's VCF heads and CVG rows share (include/basevar_amd_record_text.h): the stand-alone harness
tests/cpp/record_text_check.cpp -- host/vcf_emit.hpp's format_vcf_head and format_cvg_line, the authority for the bytes, checked
on the way against basevar_amd/csrc/bv_record_text_core.h -- built with g++ and run as a program, and seeded records to feed it."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "record_text_check.cpp")
DEPS = [SRC] + [os.path.join(ROOT, *p) for p in (("basevar_amd", "csrc", "bv_record_text_core.h"), ("basevar_amd", "csrc", "bv_numfmt_core.h"),
                                                ("basevar_amd", "host", "vcf_emit.hpp"), ("basevar_amd", "host", "batchfile.hpp"), ("include", "basevar_amd.h"))]
OUT_DIR = os.path.join(ROOT, "basevar_amd", "lib", "san")

# The tie, carry and domain-edge values of the number corpus: inside every format's domain, so that any numeric field takes them
SPECIAL = [13 / 128, 12345.25, 100000.5, 100001.5, 9.9999995, 0.9999995, 99999.95, 9.9999996, 1e-4, float(np.nextafter(1e-4, 0)), 1e-5, 1.5e-5,
           2.0 ** -40, float(np.nextafter(999999.5, 0)), 0.0, -0.0, 0.5, 2.5, 1 / 128, 3 / 128, -13 / 128, -0.0009765625, 1.0, 20.0,
           float(np.nextafter(20.0, 30.0)), 5000.0, 10000.0, 0.0009765625, 999999.4375]
# Outside one domain or another: such a record is the host's
OUTSIDE = [float("nan"), float("inf"), -float("inf"), 999999.5, float(np.nextafter(2.0 ** -40, 0)), 2.0 ** 63, 1e-300]
F6_FIELDS = ["qual", "qd", "var_sor", "var_fs", "cvg_fs", "cvg_sor"]
IOD_FIELDS = ["mq_ranksum", "rpr_ranksum", "bq_ranksum"]


def build(asan=False):
    """The harness: plain, or with ASan + UBSan (a program of its own: it needs no preloaded runtime)."""
    exe = os.path.join(OUT_DIR, "record_text_check" + (".asan" if asan else ""))
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in DEPS):
        return exe
    os.makedirs(OUT_DIR, exist_ok=True)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g"] if asan else ["-O2"]
    tmp = exe + ".%d.tmp" % os.getpid()
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")] + flags + [SRC, "-o", tmp])
    os.replace(tmp, exe)
    return exe


def record(rng, alts, n_groups=0, scale=None):
    """A seeded bv_site_result with the ALT bases `alts` (codes 0 .. 3, in order) and n_groups bv_group_result records, every
    number inside its format's domain"""
    from basevar_amd import _capi
    na = len(alts)
    r = np.zeros((), dtype=_capi.SITE_DTYPE)
    r["depth"] = rng.integers(0, 5000, 4)
    r["total_depth"] = int(r["depth"].sum()) + 1
    r["status"] = 3 if na else 1
    r["cvg_sb"] = rng.integers(0, 3000, 4)
    r["cvg_fs"], r["cvg_sor"] = rng.random() * 30, rng.random() * 8 - 4
    r["n_alt"] = na
    r["alt"][:na] = alts
    sc = 10.0 ** -int(rng.integers(0, 12)) if scale is None else scale
    r["af"][:na] = rng.random(na) * sc + 2.0 ** -40
    r["caf"][:na] = rng.random(na)
    r["qual"] = [rng.random() * 5000, rng.random() * 20, 20.0, 1e7 * rng.random()][int(rng.integers(0, 4))]
    r["qd"] = rng.random() * 40
    r["var_sb"] = rng.integers(0, 3000, 4)
    r["var_fs"], r["var_sor"] = rng.random() * 30, rng.random() * 8 - 4
    r["mq_ranksum"], r["rpr_ranksum"], r["bq_ranksum"] = rng.random(3) * 60 - 30
    g = np.zeros(n_groups, dtype=_capi.GROUP_DTYPE)
    for k in range(n_groups):
        ga = int(rng.integers(0, na + 1))  # (a group without ALT prints nothing)
        g[k]["n_alt"] = ga
        g[k]["alt"][:ga] = alts[:ga]
        g[k]["af"][:ga] = rng.random(ga) * 10.0 ** -int(rng.integers(0, 12)) + 2.0 ** -40
        g[k]["total_depth"] = int(rng.integers(0, 1000))
    return r, g


def line(rec, groups=None, chrom=b"chr1", pos=1000, ref=b"A", tokens=()):
    return dict(rec=rec, groups=groups, chrom=bytes(chrom), pos=int(pos), ref=bytes(ref), tokens=[bytes(t) for t in tokens])


def seeded_lines(seed, n, n_groups, chrom=None):
    """n lines over n_alt 0 .. 3, the special QUAL values, CHROM of 1 .. 40 bytes, lower-case REF, rows with and without indel
    tokens, depth 0"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        na = int(rng.integers(0, 4)) if k % 5 else k // 5 % 4
        alts = [int(a) for a in rng.permutation(4)[:na]]
        r, g = record(rng, alts, n_groups)
        r["qual"] = [float(r["qual"]), 0.0, 5000.0, 10000.0, 20.0, float(np.nextafter(20.0, 30.0))][k % 6]
        if k % 11 == 7:
            r["total_depth"] = 0
        if k % 13 == 5:
            r["total_depth"] = [0x7fffffff, 0x80000000, 0xffffffff][k % 3]
        tokens = []
        if k % 4 == 1:
            tokens = [[b"+AT", b"-C", b"+AT", b"-GGT", b"A", b"+ac"][int(i)] for i in rng.integers(0, 6, int(rng.integers(1, 9)))]
        c = bytes(rng.integers(48, 123, 1 + k % 40).astype(np.uint8)) if chrom is None else chrom
        out.append(line(r, g, chrom=c, pos=int(rng.integers(1, 2 ** 32 if k % 7 == 0 else 250000000)), ref=b"ACGTacgtN"[k % 9:k % 9 + 1], tokens=tokens))
    return out


def special_lines(n_groups=2):
    """The values of SPECIAL placed in every numeric field in turn (a record per value and field), and those of OUTSIDE
    likewise: the first are the device's lines, most of the second the host's"""
    rng = np.random.default_rng(77)
    out = []
    for vals in (SPECIAL, OUTSIDE):
        for v in vals:
            for f in F6_FIELDS + IOD_FIELDS + ["af0", "af2", "caf1", "gaf"]:
                if f in IOD_FIELDS and not abs(v) < 2.0 ** 31:  # (the host formatter cannot be asked for (int) of these)
                    continue
                r, g = record(rng, [2, 0, 3], n_groups, scale=1.0)
                if f == "gaf":
                    g[n_groups - 1]["n_alt"] = 2
                    g[n_groups - 1]["af"][1] = v
                elif f in ("af0", "af2", "caf1"):
                    r[f[:-1]][int(f[-1])] = v
                else:
                    r[f] = v
                out.append(line(r, g, chrom=b"chrS", pos=len(out) + 1, ref=b"C"))
    return out


def run_numbers(exe):
    p = subprocess.run([exe, "numbers"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("record_text_check numbers exit %d: %s" % (p.returncode, p.stderr.decode(errors="replace")))
    return p.stdout.decode()


def run_lines(exe, lines, group_names=(), tmp_dir="."):
    """[(on_device, gt bytes [4], VCF head, CVG row, indel column)] for `lines`: the host formatters' text.  Raises if the
    harness finds the core header and the host formatters apart on a line that is the device's."""
    parts = [struct.pack("<II", len(lines), len(group_names))]
    for g in group_names:
        parts += [struct.pack("<I", len(g)), bytes(g)]
    for ln in lines:
        parts += [struct.pack("<II", ln["pos"], len(ln["chrom"])), ln["chrom"], ln["ref"][:1], struct.pack("<I", len(ln["tokens"]))]
        for t in ln["tokens"]:
            parts += [struct.pack("<I", len(t)), t]
        parts.append(ln["rec"].tobytes())
        if group_names:
            assert ln["groups"] is not None and len(ln["groups"]) == len(group_names)
            parts.append(ln["groups"].tobytes())
    fin, fout = os.path.join(str(tmp_dir), "record_text.in"), os.path.join(str(tmp_dir), "record_text.out")
    with open(fin, "wb") as f:
        f.write(b"".join(parts))
    p = subprocess.run([exe, "lines", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("record_text_check lines exit %d: %s" % (p.returncode, p.stderr.decode(errors="replace")))
    data = open(fout, "rb").read()
    out, at = [], 0
    for _ in lines:
        on, gt = bool(data[at]), data[at + 1:at + 5]
        at += 5
        texts = []
        for _ in range(3):
            (n,) = struct.unpack_from("<I", data, at)
            texts.append(data[at + 4:at + 4 + n])
            at += 4 + n
        out.append((on, gt, texts[0], texts[1], texts[2]))
    assert at == len(data)
    return out
