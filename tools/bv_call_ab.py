#!/usr/bin/env python3
"""bv_call and bv_pileup of this build against another build's (the parent commit's) with IDENTICAL flags: the A/B for a change
to the host tools that leaves the engine alone.  Wall seconds of every run, parent and new alternated, two repeats a leg.

    python3 tools/bv_call_ab.py --parent DIR [--threads 4 16] [--repeats 2] [--out profiles/bv_call_stages_ab.txt]

DIR holds the other build's bv_call, bv_pileup and libbasevar_amd.so.  Inputs: the batchfiles of tools/gen_batchfiles.cpp
(10,000 samples, 24,000 positions) and the cohort of tools/pileup_bench.py (100 samples, depth 8, 100,000 positions, indexed with
tests/bai_py.write_bai).  Legs: batchfiles on the default route and with --inflate device --deflate device --emit device; BAM
on the default route and with --pileup device --inflate device; bv_pileup --rows device --inflate device.  The outputs of the two
builds must be the same bytes on every leg.  A leg counts as faster or slower only beyond the parent's own spread between its
repeats (best run against best run)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bai_py  # noqa: E402
import pileup_ref as pr  # noqa: E402
from pileup_bench import write_cohort  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default=os.path.join(ROOT, "basevar_amd", "lib"))
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--per-file", type=int, default=200)
    ap.add_argument("--sites", type=int, default=24000)
    ap.add_argument("--bam-samples", type=int, default=100)
    ap.add_argument("--depth", type=float, default=8.0)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--threads", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# tools/bv_call_ab.py: batchfiles %d samples in files of %d, %d positions; BAM %d samples, depth %g, %d positions (seed %d); wall seconds, "
             "parent and new alternated" % (a.samples, a.per_file, a.sites, a.bam_samples, a.depth, a.rows, a.seed)]
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "bf"))
        gen = os.path.join(d, "gen_batchfiles")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gen_batchfiles.cpp"), "-lz", "-o", gen])
        subprocess.check_call([gen, os.path.join(d, "bf"), str(a.samples), str(a.per_file), str(a.sites)], stdout=subprocess.DEVNULL)
        files = sorted(os.path.join(d, "bf", f) for f in os.listdir(os.path.join(d, "bf")) if f.endswith(".gz"))
        beg, end = 1000, 1000 + a.rows - 1
        fasta, _, bams = write_cohort(d, a.bam_samples, a.depth, beg, end, a.seed)
        for b in bams:
            bai_py.write_bai(b)
        region = "%s:%d-%d" % (pr.REF_ID, beg, end)
        bf_in = ["--batchfiles", ",".join(files), "--contig", "chr1:250000000", "--reference", "ref.fa"]
        bam_in = sum((["-I", b] for b in bams), []) + ["-R", fasta, "-q", str(pr.MAPQ_THD)]

        def call(sfx, inputs, extra):
            return lambda lib, t, tag: ([os.path.join(lib, "bv_call")] + inputs + extra + ["--thread", str(t), "--output-vcf", os.path.join(d, tag + ".vcf" + sfx),
                                                                                           "--output-cvg", os.path.join(d, tag + ".cvg" + sfx)],
                                        [".vcf" + sfx, ".cvg" + sfx])

        legs = [
            ("bv_call batchfiles, default route", call("", bf_in, [])),
            ("bv_call batchfiles --inflate device --deflate device --emit device", call(".gz", bf_in, ["--inflate", "device", "--deflate", "device", "--emit", "device"])),
            ("bv_call BAM, default route", call("", bam_in + ["-r", region], [])),
            ("bv_call BAM --pileup device --inflate device", call("", bam_in + ["-r", region], ["--pileup", "device", "--inflate", "device"])),
            ("bv_pileup --rows device --inflate device", lambda lib, t, tag: (
                [os.path.join(lib, "bv_pileup")] + bam_in + ["--regions", region, "--thread", str(t), "--rows", "device", "--inflate", "device", "-o", os.path.join(d, tag + ".bf.gz")],
                [".bf.gz"])),
        ]

        def run(cmd):
            t0 = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:  # (nothing more is started after a run that failed or ran out of time)
                raise RuntimeError(cmd[0] + ": " + p.stderr[-1500:])
            return time.perf_counter() - t0

        for name, leg in legs:
            run(leg(a.new, a.threads[0], "warm")[0])  # (file cache, first device use)
            for t in a.threads:
                par, got, same = [], [], True
                for _ in range(a.repeats):
                    cmd, outs = leg(a.parent, t, "parent")
                    par.append(run(cmd))
                    got.append(run(leg(a.new, t, "new")[0]))
                    same = same and all(open(os.path.join(d, "parent" + e), "rb").read() == open(os.path.join(d, "new" + e), "rb").read() for e in outs)
                spread, gap = max(par) - min(par), min(got) - min(par)
                verdict = "within the parent's spread" if abs(gap) <= spread else ("faster" if gap < 0 else "SLOWER")
                lines.append("  %-68s --thread %2d: parent %s (spread %.3f); new %s; best against best %+.3f s: %s; outputs identical: %s" % (
                    name, t, " ".join("%.3f" % x for x in par), spread, " ".join("%.3f" % x for x in got), gap, verdict, same))
                print(lines[-1], flush=True)
                if not same:
                    sys.exit("the outputs differ: " + name)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
