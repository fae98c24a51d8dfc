#!/usr/bin/env python3
"""`bv_call --indel-tokens device` of this build, which lists the '+SEQ' / '-SEQ' tokens of batchfile rows on the engine that
parses them, against the parent commit's binary, which fetched every marked row whole and walked it on the worker's thread --
and this build without the flag, which must do what the parent does: wall seconds of every run, alternated repeats per thread
count.  A leg counts as a gain or a loss only beyond the parent's own spread.

    python3 tools/text_tokens_ab.py --parent DIR [--bf-samples 10000 --bf-per-file 200 --bf-sites 24000 --threads 1 4 16]
                                    [--parent-flag] [--out profiles/text_tokens_bv_call_ab.txt]

  the job        tools/indel_tally_ab.py's batchfile leg: 10,000 samples in 50 BGZF files, 24,000 positions
  flag sets      --inflate device --deflate device --emit device, and --inflate device alone
DIR holds the parent commit's bv_call and libbasevar_amd.so.  The outputs of every triple are compared, inflated, before
anything is reported.  --parent-flag: the parent has the flag too and gets it -- the same flags on both sides, for a change that
must leave the speed as it is; the run without the flag is left out then."""
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
    ap.add_argument("--parent-flag", action="store_true", help="pass --indel-tokens device to the parent's binary too")
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

        def cmd(lib, t, tag, more=()):
            return [os.path.join(lib, "bv_call")] + inputs + ["--thread", str(t), "--output-vcf", os.path.join(d, tag + ".vcf.gz"), "--output-cvg",
                                                             os.path.join(d, tag + ".cvg.gz"), "--timing", os.path.join(d, tag + ".json")] + flags + list(more)
        run(cmd(new, 1, "warm"))  # (file cache, first device use)
        for t in a.threads:
            par, got, off = [], [], []
            for _ in range(a.repeats):
                par.append(run(cmd(a.parent, t, "parent", ["--indel-tokens", "device"] if a.parent_flag else [])))
                got.append(run(cmd(new, t, "new", ["--indel-tokens", "device"])))
                if not a.parent_flag:
                    off.append(run(cmd(new, t, "off")))
            tags = ("parent", "new") + (("off",) if off else ())
            same = all(len(set(digest_gz(os.path.join(d, tag + "." + x)) for tag in tags)) == 1 for x in ("vcf.gz", "cvg.gz"))
            tj, oj, pj = (json.load(open(os.path.join(d, x + ".json"))) for x in ("new", "off" if off else "new", "parent"))
            spread = max(par) - min(par)

            def verdict(best):
                return "beyond the parent's spread" if abs(min(par) - best) > spread else "within the parent's spread"
            without = "without the flag %s, %+.3f s (%s)" % (" ".join("%.3f" % x for x in off), min(off) - min(par), verdict(min(off))) if off else "the parent has the flag too"
            say("  %2d thread(s): parent %s (spread %.3f); --indel-tokens device %s, best against best %+.3f s (%s); %s; "
                "engine_s %.3f -> %.3f (flag) / %.3f (no flag), emit_s %.3f -> %.3f / %.3f; indel_tokens_device %s, text_fetch_bytes %s (flag) / %s (no flag); "
                "indel_columns_device %s, indel_columns_host %s of %d sites; outputs inflate to the same bytes: %s" % (
                    t, " ".join("%.3f" % x for x in par), spread, " ".join("%.3f" % x for x in got), min(got) - min(par), verdict(min(got)),
                    without, pj["engine_s"], tj["engine_s"], oj["engine_s"], pj["emit_s"],
                    tj["emit_s"], oj["emit_s"], tj.get("indel_tokens_device"), tj.get("text_fetch_bytes"), oj.get("text_fetch_bytes"),
                    tj.get("indel_columns_device"), tj.get("indel_columns_host"), tj["sites"], same))
            if not same:
                raise RuntimeError("the outputs differ")

    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "bf"))
        gen = os.path.join(d, "gen_batchfiles")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gen_batchfiles.cpp"), "-lz", "-o", gen])
        subprocess.check_call([gen, os.path.join(d, "bf"), str(a.bf_samples), str(a.bf_per_file), str(a.bf_sites)])
        files = sorted(os.path.join(d, "bf", f) for f in os.listdir(os.path.join(d, "bf")) if f.endswith(".gz"))
        inputs = ["--batchfiles", ",".join(files), "--contig", "chr1:250000000", "--reference", "ref.fa"]
        for flags in (["--inflate", "device", "--deflate", "device", "--emit", "device"], ["--inflate", "device"]):
            legs("tools/text_tokens_ab.py: %d samples in %d BGZF files, %d positions; --batchfiles ... %s; wall seconds" % (
                a.bf_samples, len(files), a.bf_sites, " ".join(flags)), d, inputs, flags)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
