#!/usr/bin/env python3
"""`bv_call --files-per-pass K` of this build -- the batchfiles read K at a time and every window parsed as one job
(include/basevar_amd_text_job.h) -- beside the default route, and the default route of this build against the parent commit's
binary, which it must leave as fast as it was.  Wall seconds of whole runs, two alternated repeats, best against best; a leg
counts as a gain or a loss only beyond the parent's own spread.

    python3 tools/text_job_ab.py --parent DIR [--bf-samples 10000 --bf-per-file 200 --bf-sites 24000 --threads 1 4 16]
                                 [--many-files 2000 --many-per-file 50 --many-sites 300] [--out profiles/text_job_bv_call_ab.txt]

  default route   the recorded job (10,000 samples in 50 BGZF files, 24,000 positions) without the flag: parent against new
  the new route   the same job with K = 1, 8 and 50 at the middle thread count: seconds, passes, peak RSS, max_open_batchfiles
  many files      one cohort of more files than a usual descriptor limit allows, with the flag only (the parent cannot open it
                  under that limit): positions/s and positions per window beside the 2^28 / samples rule of the default route
DIR holds the parent commit's bv_call and libbasevar_amd.so.  Outputs are compared, inflated, before anything is reported."""
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
from record_text_ab import digest_gz  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--bf-samples", type=int, default=10000)
    ap.add_argument("--bf-per-file", type=int, default=200)
    ap.add_argument("--bf-sites", type=int, default=24000)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--many-files", type=int, default=2000)
    ap.add_argument("--many-per-file", type=int, default=50)
    ap.add_argument("--many-sites", type=int, default=300)
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
        return time.perf_counter() - t0, None

    def rss_of(cmd):
        """(wall seconds, peak RSS in MiB): run as a child of a child, so that RUSAGE_CHILDREN is this run's alone"""
        code = "import resource,subprocess,sys; p=subprocess.run(sys.argv[1:],capture_output=True); print(resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss); sys.exit(p.returncode)"
        t0 = time.perf_counter()
        p = subprocess.run([sys.executable, "-c", code] + cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(" ".join(cmd[:1]) + " failed")
        return time.perf_counter() - t0, int(p.stdout.split()[-1]) / 1024.0

    with tempfile.TemporaryDirectory() as d:
        gen = os.path.join(d, "gen_batchfiles")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gen_batchfiles.cpp"), "-lz", "-o", gen])

        def cohort(name, samples, per, sites):
            os.makedirs(os.path.join(d, name))
            subprocess.check_call([gen, os.path.join(d, name), str(samples), str(per), str(sites)])
            files = sorted(os.path.join(d, name, f) for f in os.listdir(os.path.join(d, name)) if f.endswith(".gz"))
            return ["--batchfiles", ",".join(files), "--contig", "chr1:250000000", "--reference", "ref.fa"], len(files)

        def cmd(lib, inputs, t, tag, more=()):
            return [os.path.join(lib, "bv_call")] + inputs + ["--thread", str(t), "--output-vcf", os.path.join(d, tag + ".vcf.gz"), "--output-cvg",
                                                             os.path.join(d, tag + ".cvg.gz"), "--timing", os.path.join(d, tag + ".json")] + list(more)

        def same(tags):
            return all(len(set(digest_gz(os.path.join(d, tag + "." + x)) for tag in tags)) == 1 for x in ("vcf.gz", "cvg.gz"))

        inputs, F = cohort("bf", a.bf_samples, a.bf_per_file, a.bf_sites)
        say("# tools/text_job_ab.py: %d samples in %d BGZF files, %d positions; wall seconds of whole bv_call runs" % (a.bf_samples, F, a.bf_sites))
        say("## the default route (no flag): the parent commit's binary against this build's, %d alternated repeats" % a.repeats)
        run(cmd(new, inputs, 1, "warm"))
        for t in a.threads:
            par, got = [], []
            for _ in range(a.repeats):
                par.append(run(cmd(a.parent, inputs, t, "parent"))[0])
                got.append(run(cmd(new, inputs, t, "new"))[0])
            spread = max(par) - min(par)
            ok = same(("parent", "new"))
            say("  %2d thread(s): parent %s (spread %.3f); this build %s; best against best %+.3f s (%s); outputs inflate to the same bytes: %s" % (
                t, " ".join("%.3f" % x for x in par), spread, " ".join("%.3f" % x for x in got), min(got) - min(par),
                "beyond the parent's spread" if abs(min(got) - min(par)) > spread else "within the parent's spread", ok))
            if not ok:
                raise RuntimeError("the outputs differ")
        t = a.threads[len(a.threads) // 2]
        say("## the new route, %d threads: --files-per-pass K against this build's default route (best of %d)" % (t, a.repeats))
        base = min(rss_of(cmd(new, inputs, t, "new")) for _ in range(a.repeats))
        bj = json.load(open(os.path.join(d, "new.json")))
        say("  default route        %.3f s, peak RSS %.0f MiB, batches of %d sites" % (base[0], base[1], bj["batch_sites"]))
        for K in (1, 8, 50):
            got = min(rss_of(cmd(new, inputs, t, "k%d" % K, ["--files-per-pass", str(K)])) for _ in range(a.repeats))
            j = json.load(open(os.path.join(d, "k%d.json" % K)))
            ok = same(("new", "k%d" % K))
            say("  --files-per-pass %-3d %.3f s (%.2f x the default route), peak RSS %.0f MiB, windows of %d sites, passes %d, max_open_batchfiles %d; "
                "engine_s %.3f emit_s %.3f; outputs inflate to the same bytes: %s" % (
                    K, got[0], got[0] / base[0], got[1], j["batch_sites"], j["passes"], j["max_open_batchfiles"], j["engine_s"], j["emit_s"], ok))
            if not ok:
                raise RuntimeError("the outputs differ")
        if a.many_files:
            n = a.many_files * a.many_per_file
            inputs, F = cohort("many", n, a.many_per_file, a.many_sites)
            say("## many files: %d samples in %d BGZF files of %d, %d positions; the flag only (soft RLIMIT_NOFILE here: %d)" % (
                n, F, a.many_per_file, a.many_sites, __import__("resource").getrlimit(__import__("resource").RLIMIT_NOFILE)[0]))
            for K in (64, 256):
                got = rss_of(cmd(new, inputs, t, "many%d" % K, ["--files-per-pass", str(K)]))
                j = json.load(open(os.path.join(d, "many%d.json" % K)))
                say("  --files-per-pass %-3d %.3f s, %.1f positions/s, peak RSS %.0f MiB, windows of %d positions (the default route's rule, 2^28 / samples: %d; "
                    "its text blocks: half of that), passes %d, max_open_batchfiles %d" % (
                        K, got[0], j["sites"] / got[0], got[1], j["batch_sites"], (1 << 28) // n, j["passes"], j["max_open_batchfiles"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
