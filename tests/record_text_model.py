"""A serial restatement in Python of the VCF head and the CVG row that basevar_amd/csrc/bv_record_text_core.h defines, written
from that header's definition and sharing no code with it: the numbers go through Python's own "%f" / "%g" / "%d", which are
correctly rounded, and the lines are put together field by field.  The tests hold the stand-alone harness's dump
(tests/cpp/record_text_check.cpp: the host formatters' text) and the device's text to it."""
import math

BASES = "ACGT"
MAX_ALT = 3  # ALTs of a record that the device formats


def f6_ok(v):
    return math.isfinite(v) and abs(v) < 2.0 ** 63


def g6_ok(v):
    return v == 0 or (math.isfinite(v) and 2.0 ** -40 <= abs(v) < 999999.5)


def iod_ok(v):
    return math.isfinite(v) and abs(v) < 2.0 ** 31


def f6(v):
    return "%f" % v


def g6(v):
    return "%g" % v


def iod(v):
    return "%d" % int(v)  # truncation toward zero; "0" for -0.5


def i32(u):
    u = int(u)
    return "%d" % (u - (1 << 32) if u >= (1 << 31) else u)


def on_device(r, groups=()):
    """Is every number the two lines of record `r` print inside its format's domain (and are its ALTs at most three)?"""
    if int(r["n_alt"]) > MAX_ALT or any(int(g["n_alt"]) > MAX_ALT for g in groups):
        return False
    if int(r["total_depth"]) != 0 and not (f6_ok(float(r["cvg_fs"])) and f6_ok(float(r["cvg_sor"]))):
        return False
    na = int(r["n_alt"])
    if na == 0:
        return True
    ok = all(f6_ok(float(r[k])) for k in ("qual", "qd", "var_sor", "var_fs"))
    ok = ok and all(iod_ok(float(r[k])) for k in ("mq_ranksum", "rpr_ranksum", "bq_ranksum"))
    ok = ok and all(g6_ok(float(r["af"][i])) and g6_ok(float(r["caf"][i])) for i in range(na))
    return ok and all(g6_ok(float(g["af"][i])) for g in groups for i in range(int(g["n_alt"])))


def vcf_head(r, groups, group_names, chrom, pos, ref):
    """CHROM through FORMAT of record `r` (bytes); b"" without ALT.  `ref`: one byte, letter case kept."""
    na = int(r["n_alt"])
    if na == 0:
        return b""
    alts = [int(a) & 3 for a in r["alt"][:na]]
    qual = float(r["qual"])
    info = ["CM_DP=" + i32(r["total_depth"]),
            "CM_AC=" + ",".join(i32(r["depth"][a]) for a in alts),
            "CM_AF=" + ",".join(g6(float(v)) for v in r["af"][:na]),
            "CM_CAF=" + ",".join(g6(float(v)) for v in r["caf"][:na]),
            "MQRankSum=" + iod(float(r["mq_ranksum"])),
            "ReadPosRankSum=" + iod(float(r["rpr_ranksum"])),
            "BaseQRankSum=" + iod(float(r["bq_ranksum"])),
            "QD=" + f6(float(r["qd"])),
            "SOR=" + f6(float(r["var_sor"])),
            "FS=" + f6(float(r["var_fs"])),
            "SB_REF=%s,%s" % (i32(r["var_sb"][0]), i32(r["var_sb"][1])),
            "SB_ALT=%s,%s" % (i32(r["var_sb"][2]), i32(r["var_sb"][3]))]
    for g, name in zip(groups, group_names):
        if int(g["n_alt"]):
            info.append(bytes(name).decode("latin-1") + "_AF=" + ",".join(g6(float(v)) for v in g["af"][:int(g["n_alt"])]))
    cols = [bytes(chrom).decode("latin-1"), "%d" % int(pos), ".", bytes(ref).decode("latin-1"), ",".join(BASES[a] for a in alts), f6(qual),
            "." if qual > 20 else "LowQual", ";".join(info), "GT:AB:SO:BP"]
    return "\t".join(cols).encode("latin-1")


def cvg_row(r, chrom, pos, ref, indel=b""):
    """The CVG row of record `r` with its line break (bytes); b"" at depth 0.  `indel`: the row's indel column, empty: "." """
    if int(r["total_depth"]) == 0:
        return b""
    cols = [bytes(chrom).decode("latin-1"), "%d" % int(pos), bytes(ref).decode("latin-1"), i32(r["total_depth"])]
    cols += [i32(d) for d in r["depth"]]
    cols += [bytes(indel).decode("latin-1") or ".", f6(float(r["cvg_fs"])), f6(float(r["cvg_sor"])), ",".join(i32(c) for c in r["cvg_sb"])]
    return ("\t".join(cols) + "\n").encode("latin-1")


def gt_codes(r, ref):
    """uint8 [4]: per base A, C, G, T the character '0' (the REF base), '1' .. (the ALT of that number) or '.'"""
    up = bytes(ref).decode("latin-1").upper()
    out = [ord("0") if b == up else ord(".") for b in BASES]
    for i in range(int(r["n_alt"])):
        a = int(r["alt"][i]) & 3
        if BASES[a] != up:
            out[a] = ord("1") + i
    return bytes(out)


def indel_column(tokens):
    """The sorted "TOKEN|count" tally of a row's '+' / '-' tokens (bytes), b"." without any"""
    tally = {}
    for t in tokens:
        t = bytes(t)
        if t and t[:1] not in (b"N", b"A", b"C", b"G", b"T"):
            tally[t] = tally.get(t, 0) + 1
    return b",".join(k + b"|" + str(tally[k]).encode() for k in sorted(tally)) or b"."
