#!/usr/bin/env python3
"""`bv_call --batchfiles ... --regions` on the recorded 10,000-sample x 24,000-position batchfile job (the generator that
tools/text_tokens_ab.py uses; it writes a .tbi beside every file): what a region of one tenth of the positions costs beside the
whole-file run, whether the run without --regions still does what the parent commit's binary does, and the selection kernels'
time beside the row parser's.

    python3 tools/batchfile_regions_ab.py --parent DIR [--bf-samples 10000 --bf-per-file 200 --bf-sites 24000 --threads 1 4 16]
                                          [--legs region unchanged kernels] [--no-kernels] [--out profiles/batchfile_regions_ab.txt]

  region leg          a region of one tenth of the positions in the middle, under --inflate host and --inflate device, against the
                      same build's whole-file run: seconds, members read against members in the files, and the fixed cost that does not shrink with the
                      region (the region run's seconds minus a tenth of the whole run's)
  unchanged-path leg  the whole-file run without --regions, under both, against DIR's bv_call (the parent commit's binary and library): two
                      alternated repeats, best against best; a leg counts only beyond the parent's own spread
  kernels alone       one `rocprofv3 --kernel-trace --stats` run of the region call (no counters): the selection kernels' and
                      bv_text_parse_kernel's calls and time
members read are counted by --inflate device alone (the host reader's --timing has no such figure)."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
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
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--legs", nargs="+", default=["region", "unchanged", "kernels"], help="which of the legs to run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    new = os.path.join(ROOT, "basevar_amd", "lib")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(cmd, wrap=()):
        t0 = time.perf_counter()
        p = subprocess.run(list(wrap) + cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(" ".join(cmd[:1]) + ": " + p.stderr[-1500:])
        return time.perf_counter() - t0

    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "bf"))
        gen = os.path.join(d, "gen_batchfiles")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gen_batchfiles.cpp"), "-lz", "-o", gen])
        subprocess.check_call([gen, os.path.join(d, "bf"), str(a.bf_samples), str(a.bf_per_file), str(a.bf_sites)])
        files = sorted(os.path.join(d, "bf", f) for f in os.listdir(os.path.join(d, "bf")) if f.endswith(".gz"))
        inputs = ["--batchfiles", ",".join(files), "--contig", "chr1:250000000", "--reference", "ref.fa"]
        first = 1000 + a.bf_sites * 9 // 20
        region = "chr1:%d-%d" % (first, first + a.bf_sites // 10 - 1)

        def cmd(lib, t, tag, more=()):
            return [os.path.join(lib, "bv_call")] + inputs + ["--thread", str(t), "--output-vcf", os.path.join(d, tag + ".vcf.gz"), "--output-cvg",
                                                             os.path.join(d, tag + ".cvg.gz"), "--timing", os.path.join(d, tag + ".json")] + list(more)
        run(cmd(new, 1, "warm", ["--inflate", "device"]))  # (file cache, first device use)
        say("# tools/batchfile_regions_ab.py: %d samples in %d BGZF files, %d positions; *.gz outputs; wall seconds" % (a.bf_samples, len(files), a.bf_sites))
        say("# region leg: --regions %s (one tenth of the positions, in the middle) against the same build's whole-file run" % region)
        for inflate, t in [(i, t) for i in ("host", "device") for t in a.threads] if "region" in a.legs else []:
            whole, part = [], []
            for _ in range(a.repeats):
                whole.append(run(cmd(new, t, "whole", ["--inflate", inflate])))
                part.append(run(cmd(new, t, "region", ["--inflate", inflate, "--regions", region])))
            wj, rj = json.load(open(os.path.join(d, "whole.json"))), json.load(open(os.path.join(d, "region.json")))
            members = "members read %d -> %d of %d in the files; " % (wj["members_inflated"], rj["members_inflated"], wj["members_in_files"]) if inflate == "device" else ""
            say("  --inflate %-6s %2d thread(s): whole %s, region %s; best %.3f -> %.3f s; fixed cost (region - whole / 10) %.3f s; sites %d -> %d; "
                "%sengine_s %.3f -> %.3f, read_s %.3f -> %.3f, emit_s %.3f -> %.3f" % (
                    inflate, t, " ".join("%.3f" % x for x in whole), " ".join("%.3f" % x for x in part), min(whole), min(part), min(part) - min(whole) / 10,
                    wj["sites"], rj["sites"], members, wj["engine_s"], rj["engine_s"], wj["read_s"], rj["read_s"], wj["emit_s"], rj["emit_s"]))
        say("# unchanged-path leg: the whole-file run without --regions against the parent commit's binary")
        for inflate, t in [(i, t) for i in ("host", "device") for t in a.threads] if "unchanged" in a.legs else []:
            par, got = [], []
            for _ in range(a.repeats):
                par.append(run(cmd(a.parent, t, "parent", ["--inflate", inflate])))
                got.append(run(cmd(new, t, "new", ["--inflate", inflate])))
            same = all(digest_gz(os.path.join(d, "parent." + x)) == digest_gz(os.path.join(d, "new." + x)) for x in ("vcf.gz", "cvg.gz"))
            spread = max(par) - min(par)
            say("  --inflate %-6s %2d thread(s): parent %s (spread %.3f); this build %s; best against best %+.3f s (%s the parent's spread); outputs inflate to the same bytes: %s" % (
                inflate, t, " ".join("%.3f" % x for x in par), spread, " ".join("%.3f" % x for x in got), min(got) - min(par),
                "beyond" if abs(min(got) - min(par)) > spread else "within", same))
            if not same:
                raise RuntimeError("the outputs differ")
        if "kernels" not in a.legs:
            pass
        elif not a.no_kernels and shutil.which("rocprofv3"):
            prof = os.path.join(d, "prof")
            run(cmd(new, 4, "prof", ["--inflate", "device", "--regions", region]), wrap=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--"])
            rows = []
            for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
                rows += list(csv.DictReader(open(f)))
            say("# kernels alone: one rocprofv3 --kernel-trace --stats run of the region call at 4 threads (name: calls, total us, average us)")
            for r in rows:
                if any(w in r["Name"] for w in ("bv_text_region_", "bv_text_parse_kernel", "bv_text_line_", "bv_inflate")):
                    say("  %s: %s calls, %.1f us, %.2f us each" % (re.search(r"bv_\w+", r["Name"]).group(0), r["Calls"], float(r["TotalDurationNs"]) / 1e3, float(r["AverageNs"]) / 1e3))
            if not rows:
                say("  (no kernel statistics came out of the run: not measured)")
        else:
            say("# kernels alone: not measured (no rocprofv3 run)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
