#!/usr/bin/env python3
"""`bv_pileup --rows device` of this build against `bv_pileup` of another build (the parent commit's) on a synthetic BAM cohort:
the 10,000-sample shape of tools/pileup_bench.py (depth 0.5, 13,000 rows), a `.gz` batchfile out.

    python3 tools/pileup_text_ab.py --parent DIR_WITH_bv_pileup [--new basevar_amd/lib] [--samples 10000] [--depth 0.5]
                                    [--rows 13000] [--threads 1 4 16] [--repeats 2] [--levels fast] [--work DIR] [--out FILE]

Writes the cohort with tools/pileup_bench.py's writer, then for every thread count and every repeat runs the parent and the new
leg one after the other (alternated), checks that the two outputs inflate to the same bytes, and prints each run's wall seconds
and a summary.  A leg counts as faster or slower only where the gap exceeds the parent's own spread between its repeats."""
import argparse
import gzip
import hashlib
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


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
    ap.add_argument("--depth", type=float, default=0.5)
    ap.add_argument("--rows", type=int, default=13000)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--levels", nargs="+", default=["fast"])
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pileup_bench
    import pileup_ref as pr
    work = a.work or tempfile.mkdtemp(prefix="pileup_text_ab_")
    os.makedirs(os.path.join(work, "bam"), exist_ok=True)
    beg, end = 1000, 1000 + a.rows - 1
    fasta, _, bams = pileup_bench.write_cohort(os.path.join(work, "bam"), a.samples, a.depth, beg, end, 77)
    lst = os.path.join(work, "bams.list")
    with open(lst, "w") as f:
        f.write("".join(b + "\n" for b in bams))
    region = "%s:%d-%d" % (pr.REF_ID, beg, end)
    lines = ["== bv_pileup A/B: %d samples (depth %g), %s, .gz batchfile out, --filename-has-samplename; parent = the parent commit's bv_pileup; new = this "
             "build with --rows device" % (a.samples, a.depth, region)]
    print(lines[0], flush=True)

    def run(tag, exe, threads, extra):
        out = os.path.join(work, tag + ".bf.gz")
        t0 = time.perf_counter()
        p = subprocess.run([os.path.join(exe, "bv_pileup"), "-R", fasta, "--regions", region, "-q", str(pr.MAPQ_THD), "-L", lst, "--filename-has-samplename",
                            "--thread", str(threads), "-o", out] + extra, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        if p.returncode != 0:
            sys.exit("%s failed (%d): %s" % (tag, p.returncode, p.stderr[-2000:]))
        return out, dt

    want = None
    for t in a.threads:
        legs = {"parent": []}
        for level in a.levels:
            legs["device " + level] = []
        for r in range(a.repeats):
            out, dt = run("parent", a.parent, t, [])
            legs["parent"].append(dt)
            if want is None:
                want = digest_gz(out)
                lines.append("inflated output: %d bytes of .gz from the parent, sha256 %s" % (os.path.getsize(out), want[:16]))
            for level in a.levels:
                out, dt = run("new_" + level, a.new, t, ["--rows", "device", "--deflate-level", level])
                if r == 0:
                    assert digest_gz(out) == want, "the device route's batchfile inflates to other bytes"
                    lines.append("  --thread %d --deflate-level %s: inflates to the parent's bytes, %d bytes of .gz" % (t, level, os.path.getsize(out)))
                legs["device " + level].append(dt)
        spread = max(legs["parent"]) - min(legs["parent"])
        for name, ts in legs.items():
            verdict = ""
            if name != "parent":
                verdict = "  FASTER" if max(ts) < min(legs["parent"]) - spread else "  SLOWER" if min(ts) > max(legs["parent"]) + spread else "  within the parent's spread"
            lines.append("--thread %-2d %-13s wall %s s%s" % (t, name, " / ".join("%.2f" % x for x in ts), verdict))
        print("\n".join(lines[-(len(legs) + len(a.levels)):]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
