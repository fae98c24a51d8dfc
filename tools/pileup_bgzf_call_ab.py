#!/usr/bin/env python3
"""`bv_call --pileup device --inflate device` and `bv_pileup --rows device --inflate device` against a parent build's
`--pileup device` / `--rows device` alone, on a seeded cohort of tools/pileup_bench.py (indexed with tests/bai_py.write_bai):
wall seconds of every run, two alternated repeats per thread count.  A leg counts only beyond the parent's own spread.

    python3 tools/pileup_bgzf_call_ab.py --parent DIR [--samples 100 --depth 8 --rows 100000 --threads 1 4 16] [--out profiles/pileup_bgzf_bv_call_ab.txt]

DIR holds the parent commit's bv_call, bv_pileup and libbasevar_amd.so (a build of the parent tree's basevar_amd/lib)."""
import argparse
import json
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
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--depth", type=float, default=8.0)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    new = os.path.join(ROOT, "basevar_amd", "lib")
    beg, end = 1000, 1000 + a.rows - 1
    lines = ["# tools/pileup_bgzf_call_ab.py --samples %d --depth %g --rows %d (region %s:%d-%d, indexed files, seed %d); wall seconds" % (
        a.samples, a.depth, a.rows, pr.REF_ID, beg, end, a.seed)]
    with tempfile.TemporaryDirectory() as d:
        fasta, fa, bams = write_cohort(d, a.samples, a.depth, beg, end, a.seed)
        for b in bams:
            bai_py.write_bai(b)
        inputs = sum((["-I", b] for b in bams), [])
        region = "%s:%d-%d" % (pr.REF_ID, beg, end)

        def run(cmd):
            t0 = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                raise RuntimeError(" ".join(cmd[:1]) + ": " + p.stderr[-1500:])
            return time.perf_counter() - t0

        legs = {
            "bv_call": lambda lib, t, extra, tag: [os.path.join(lib, "bv_call")] + inputs + ["-R", fasta, "-r", region, "-q", str(pr.MAPQ_THD), "--thread", str(t), "--pileup", "device",
                                                    "--output-vcf", os.path.join(d, tag + ".vcf"), "--output-cvg", os.path.join(d, tag + ".cvg"), "--timing", os.path.join(d, tag + ".json")] + extra,
            "bv_pileup": lambda lib, t, extra, tag: [os.path.join(lib, "bv_pileup")] + inputs + ["-R", fasta, "--regions", region, "-q", str(pr.MAPQ_THD), "--thread", str(t), "--rows", "device",
                                                      "-o", os.path.join(d, tag + ".bf.gz")] + extra,
        }
        for tool, cmd in legs.items():
            run(cmd(new, 1, ["--inflate", "device"], "warm"))  # (file cache, first device use)
            for t in a.threads:
                par, got = [], []
                for rep in range(a.repeats):
                    par.append(run(cmd(a.parent, t, [], "parent")))
                    got.append(run(cmd(new, t, ["--inflate", "device"], "new")))
                same = all(open(os.path.join(d, "parent" + e), "rb").read() == open(os.path.join(d, "new" + e), "rb").read() for e in ((".vcf", ".cvg") if tool == "bv_call" else ()))
                more = ""
                if tool == "bv_call":
                    tj = json.load(open(os.path.join(d, "new.json")))
                    more = "; members_inflated %d, members_bytes %d; outputs identical: %s" % (tj["members_inflated"], tj["members_bytes"], same)
                spread = max(par) - min(par)
                gain = min(par) - min(got)
                lines.append("  %-9s %2d thread(s): parent %s (spread %.3f); --inflate device %s; best against best %+.3f s (%s)%s" % (
                    tool, t, " ".join("%.3f" % x for x in par), spread, " ".join("%.3f" % x for x in got), -gain,
                    "beyond the parent's spread" if abs(gain) > spread else "within the parent's spread", more))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
