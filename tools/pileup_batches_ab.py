#!/usr/bin/env python3
"""`bv_pileup -B N --rows device --batches-per-pass K` of this build against one `bv_pileup --rows device` run per batch of another
build (the parent commit's), on the 10,000-sample synthetic BAM cohort of tools/pileup_bench.py (depth 0.5, 13,000 rows), `.gz`
batchfiles out; and this build's `bv_pileup --rows device` WITHOUT -B against the parent's, the path that must not change.

    python3 tools/pileup_batches_ab.py --parent DIR_WITH_bv_pileup [--new basevar_amd/lib] [--samples 10000] [--batch 200]
                                       [--per-pass 1 4 16 50] [--threads 1 16] [--repeats 2] [--work DIR] [--out FILE]

For every thread count and every repeat the legs run one after the other (alternated).  The first run of every -B leg is checked:
each of its files inflates to the bytes of the parent's run over that batch.  A leg counts as faster or slower than another only
where the gap exceeds the parent legs' own spread between their repeats.  The cohort's windows cover whole files (13,000 rows), so
this cannot show what a shorter window -- more batches a pass -- costs in repeated member reads on real low-pass BAM files."""
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
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--depth", type=float, default=0.5)
    ap.add_argument("--rows", type=int, default=13000)
    ap.add_argument("--per-pass", type=int, nargs="+", default=[1, 4, 16, 50])
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pileup_bench
    import pileup_ref as pr
    work = a.work or tempfile.mkdtemp(prefix="pileup_batches_ab_")
    os.makedirs(os.path.join(work, "bam"), exist_ok=True)
    beg, end = 1000, 1000 + a.rows - 1
    fasta, _, bams = pileup_bench.write_cohort(os.path.join(work, "bam"), a.samples, a.depth, beg, end, 77)
    n_files = (a.samples + a.batch - 1) // a.batch
    lists = []
    for j in range(n_files + 1):  # list 0: all samples; list j: batch j
        lst = os.path.join(work, "bams_%d.list" % j)
        with open(lst, "w") as f:
            f.write("".join(b + "\n" for b in (bams if j == 0 else bams[(j - 1) * a.batch:j * a.batch])))
        lists.append(lst)
    region = "%s:%d-%d" % (pr.REF_ID, beg, end)
    lines = ["== bv_pileup -B A/B: %d samples (depth %g) in batches of %d = %d files, %s, .gz out, --filename-has-samplename, --rows device everywhere"
             % (a.samples, a.depth, a.batch, n_files, region)]
    print(lines[0], flush=True)

    def run(exe, lst, threads, out, extra):
        t0 = time.perf_counter()
        p = subprocess.run([os.path.join(exe, "bv_pileup"), "-R", fasta, "--regions", region, "-q", str(pr.MAPQ_THD), "-L", lst, "--filename-has-samplename",
                            "--thread", str(threads), "--rows", "device", "-o", out] + extra, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        if p.returncode != 0:
            sys.exit("%s failed (%d): %s" % (out, p.returncode, p.stderr[-2000:]))
        return dt

    want = None
    for t in a.threads:
        legs = {"parent, %d runs" % n_files: [], "parent, no -B": [], "new, no -B": []}
        for k in a.per_pass:
            legs["new -B, K = %d" % k] = []
        for r in range(a.repeats):
            dt = 0.0
            for j in range(1, n_files + 1):
                dt += run(a.parent, lists[j], t, os.path.join(work, "parent.%d_%d.bf.gz" % (j, n_files)), [])
            legs["parent, %d runs" % n_files].append(dt)
            if want is None:
                want = [digest_gz(os.path.join(work, "parent.%d_%d.bf.gz" % (j, n_files))) for j in range(1, n_files + 1)]
            for k in a.per_pass:
                legs["new -B, K = %d" % k].append(run(a.new, lists[0], t, os.path.join(work, "new"), ["-B", str(a.batch), "--batches-per-pass", str(k)]))
                if r == 0:
                    got = [digest_gz(os.path.join(work, "new.%d_%d.bf.gz" % (j, n_files))) for j in range(1, n_files + 1)]
                    assert got == want, "a -B file inflates to other bytes than the parent's run over its batch"
                    lines.append("  --thread %d K = %d: all %d files inflate to the parent's bytes" % (t, k, n_files))
            legs["parent, no -B"].append(run(a.parent, lists[0], t, os.path.join(work, "parent_all.bf.gz"), []))
            legs["new, no -B"].append(run(a.new, lists[0], t, os.path.join(work, "new_all.bf.gz"), []))
            if r == 0:
                assert digest_gz(os.path.join(work, "parent_all.bf.gz")) == digest_gz(os.path.join(work, "new_all.bf.gz"))
        for name, ts in legs.items():
            lines.append("--thread %-2d %-18s wall %s s   (spread %.2f)" % (t, name, " / ".join("%.2f" % x for x in ts), max(ts) - min(ts)))
        print("\n".join(lines[-(len(legs) + len(a.per_pass)):]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
