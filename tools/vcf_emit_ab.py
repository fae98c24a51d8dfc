#!/usr/bin/env python3
"""`bv_call --emit device --deflate device` of this build against `bv_call --deflate device` of another build (the parent
commit's), on synthetic reference-format batchfiles: the job of profiles/bgzf_deflate_bv_call_ab.txt.

    python3 tools/vcf_emit_ab.py --parent DIR_WITH_bv_call [--new basevar_amd/lib] [--samples 10000] [--per-file 200]
                                 [--sites 24000] [--threads 1 4 16] [--repeats 2] [--work DIR]

Writes the batchfiles with tools/gen_batchfiles.cpp, then for --inflate host and --inflate device, every thread count and
every repeat runs the parent and the new leg one after the other (alternated), checks that the two *.vcf.gz inflate to the
same bytes and that the *.cvg.gz are the same file, and prints each run's --timing line and a summary of total_s.  A leg
counts as faster or slower only where the gap exceeds the parent's own spread between its repeats."""
import argparse
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest_gz(path):
    h = hashlib.sha256()
    with gzip.open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default=os.path.join(ROOT, "basevar_amd", "lib"))
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--per-file", type=int, default=200)
    ap.add_argument("--sites", type=int, default=24000)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="vcf_emit_ab_")
    os.makedirs(os.path.join(work, "bf"), exist_ok=True)
    gen = os.path.join(work, "gen_batchfiles")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gen_batchfiles.cpp"), "-lz", "-o", gen])
    subprocess.check_call([gen, os.path.join(work, "bf"), str(a.samples), str(a.per_file), str(a.sites)])
    files = sorted(os.path.join(work, "bf", f) for f in os.listdir(os.path.join(work, "bf")) if f.endswith(".gz"))
    print("== bv_call A/B: %d samples in %d BGZF files of %d, %d positions, .vcf.gz / .cvg.gz outputs; parent = the parent commit's bv_call "
          "--deflate device; new = this build with --emit device --deflate device" % (a.samples, len(files), a.per_file, a.sites), flush=True)

    def run(tag, exe, extra):
        v, c, t = (os.path.join(work, tag + sfx) for sfx in (".vcf.gz", ".cvg.gz", ".json"))
        p = subprocess.run([os.path.join(exe, "bv_call"), "--batchfiles", ",".join(files), "--output-vcf", v, "--output-cvg", c, "--timing", t,
                            "--contig", "chr1:250000000", "--reference", "ref.fa", "--deflate", "device"] + extra, capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit("%s failed (%d): %s" % (tag, p.returncode, p.stderr[-2000:]))
        return v, c, json.load(open(t))

    totals = {}
    for inflate in ("host", "device"):
        for rep in range(1, a.repeats + 1):
            for th in a.threads:
                common = ["--inflate", inflate, "--thread", str(th)]
                old = run("parent", a.parent, common)
                new = run("new", a.new, common + ["--emit", "device"])
                for name, r in (("parent", old), ("new", new)):
                    print("%s inflate=%s thread=%d rep=%d %s" % (name, inflate, th, rep, json.dumps(r[2])), flush=True)
                    totals.setdefault((inflate, th, name), []).append(r[2])
                same_vcf = digest_gz(old[0]) == digest_gz(new[0])
                same_cvg = open(old[1], "rb").read() == open(new[1], "rb").read()
                print("  vcf.gz inflates to the same bytes: %s; cvg.gz byte-identical: %s; vcf.gz parent %d B, new %d B; vcf_lines_device %s of %d records"
                      % (same_vcf, same_cvg, os.path.getsize(old[0]), os.path.getsize(new[0]), new[2].get("vcf_lines_device"), new[2]["vcf_records"]), flush=True)
                if not (same_vcf and same_cvg):
                    sys.exit("the outputs differ")
    print("\n== summary (total_s of the repeats; engine_s is summed over the three workers, emit_s is the emitter thread)")
    for inflate in ("host", "device"):
        for th in a.threads:
            old, new = totals[(inflate, th, "parent")], totals[(inflate, th, "new")]
            o, n = [r["total_s"] for r in old], [r["total_s"] for r in new]
            spread = max(o) - min(o)
            gap = sum(o) / len(o) - sum(n) / len(n)
            verdict = "within the parent's spread" if abs(gap) <= spread else ("faster" if gap > 0 else "SLOWER")
            fmt = lambda xs: " / ".join("%.2f" % x for x in xs)
            print("--inflate %-6s --thread %2d: parent %s s   --emit device %s s   (parent's spread %.2f s, gap %+.2f s: %s)"
                  % (inflate, th, fmt(o), fmt(n), spread, gap, verdict))
            print("     engine_s: parent %s   new %s;   emit_s: parent %s   new %s" % (fmt([r["engine_s"] for r in old]), fmt([r["engine_s"] for r in new]),
                                                                                          fmt([r["emit_s"] for r in old]), fmt([r["emit_s"] for r in new])))


if __name__ == "__main__":
    main()
