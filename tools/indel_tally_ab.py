#!/usr/bin/env python3
"""`bv_call --emit device` of this build, which tallies the CVG rows' indel columns on the engine, against the parent commit's
binary with the same flags, which tallied them on the host (one std::map a row) and fetched every window's tokens to do so:
wall seconds of every run, alternated repeats per thread count.  A leg counts only beyond the parent's own spread.

    python3 tools/indel_tally_ab.py --parent DIR [--samples 100 --depth 8 --rows 100000 --threads 1 4 16]
                                    [--bf-samples 10000 --bf-per-file 200 --bf-sites 24000] [--out profiles/indel_tally_bv_call_ab.txt]

  BAM leg        the 100-sample cohort of tools/record_text_ab.py: -I ... --pileup device --inflate device --deflate device --emit device
  batchfile leg  its 10,000-sample job: --batchfiles ... --inflate device --deflate device --emit device
DIR holds the parent commit's bv_call and libbasevar_amd.so.  The outputs of every pair are compared before anything is reported."""
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
from record_text_ab import digest_gz  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--depth", type=float, default=8.0)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--bf-samples", type=int, default=10000)
    ap.add_argument("--bf-per-file", type=int, default=200)
    ap.add_argument("--bf-sites", type=int, default=24000)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--skip", choices=["bam", "batchfile"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    new = os.path.join(ROOT, "basevar_amd", "lib")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(cmd):
        t0 = time.perf_counter()
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(" ".join(cmd[:1]) + ": " + p.stderr[-1500:])
        return time.perf_counter() - t0

    def legs(title, d, inputs, flags):
        say("# " + title)

        def cmd(lib, t, tag):
            return [os.path.join(lib, "bv_call")] + inputs + ["--thread", str(t), "--output-vcf", os.path.join(d, tag + ".vcf.gz"), "--output-cvg",
                                                             os.path.join(d, tag + ".cvg.gz"), "--timing", os.path.join(d, tag + ".json")] + flags
        run(cmd(new, 1, "warm"))  # (file cache, first device use)
        for t in a.threads:
            par, got = [], []
            for _ in range(a.repeats):
                par.append(run(cmd(a.parent, t, "parent")))
                got.append(run(cmd(new, t, "new")))
            same = digest_gz(os.path.join(d, "parent.vcf.gz")) == digest_gz(os.path.join(d, "new.vcf.gz")) and \
                digest_gz(os.path.join(d, "parent.cvg.gz")) == digest_gz(os.path.join(d, "new.cvg.gz"))
            tj, pj = json.load(open(os.path.join(d, "new.json"))), json.load(open(os.path.join(d, "parent.json")))
            spread, gain = max(par) - min(par), min(par) - min(got)
            say("  %2d thread(s): parent %s (spread %.3f); this build %s; best against best %+.3f s (%s); engine_s %.3f -> %.3f, parse_pack_s %.3f -> %.3f, "
                "emit_s %.3f -> %.3f; indel_columns_device %s, indel_columns_host %s, cvg_lines_device %s of %d sites; outputs inflate to the same bytes: %s" % (
                    t, " ".join("%.3f" % x for x in par), spread, " ".join("%.3f" % x for x in got), -gain,
                    "beyond the parent's spread" if abs(gain) > spread else "within the parent's spread", pj["engine_s"], tj["engine_s"], pj["parse_pack_s"],
                    tj["parse_pack_s"], pj["emit_s"], tj["emit_s"], tj.get("indel_columns_device"), tj.get("indel_columns_host"), tj.get("cvg_lines_device"), tj["sites"], same))
            if not same:
                raise RuntimeError("the outputs differ")

    with tempfile.TemporaryDirectory() as d:
        if a.skip != "bam":
            beg, end = 1000, 1000 + a.rows - 1
            fasta, fa, bams = write_cohort(d, a.samples, a.depth, beg, end, a.seed)
            for b in bams:
                bai_py.write_bai(b)
            legs("tools/indel_tally_ab.py BAM leg: %d samples, depth %g, region %s:%d-%d (indexed files, seed %d); -I ... --pileup device --inflate device "
                 "--deflate device --emit device; wall seconds" % (a.samples, a.depth, pr.REF_ID, beg, end, a.seed), d,
                 sum((["-I", b] for b in bams), []) + ["-R", fasta, "-r", "%s:%d-%d" % (pr.REF_ID, beg, end), "-q", str(pr.MAPQ_THD)],
                 ["--pileup", "device", "--inflate", "device", "--deflate", "device", "--emit", "device"])
        if a.skip != "batchfile":
            os.makedirs(os.path.join(d, "bf"))
            gen = os.path.join(d, "gen_batchfiles")
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gen_batchfiles.cpp"), "-lz", "-o", gen])
            subprocess.check_call([gen, os.path.join(d, "bf"), str(a.bf_samples), str(a.bf_per_file), str(a.bf_sites)])
            files = sorted(os.path.join(d, "bf", f) for f in os.listdir(os.path.join(d, "bf")) if f.endswith(".gz"))
            legs("tools/indel_tally_ab.py batchfile leg: %d samples in %d BGZF files, %d positions; --batchfiles ... --inflate device --deflate device "
                 "--emit device; wall seconds" % (a.bf_samples, len(files), a.bf_sites), d,
                 ["--batchfiles", ",".join(files), "--contig", "chr1:250000000", "--reference", "ref.fa"], ["--inflate", "device", "--deflate", "device", "--emit", "device"])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
