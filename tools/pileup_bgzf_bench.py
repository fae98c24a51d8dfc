#!/usr/bin/env python3
"""What does inflating the BAM members on the device gain?  The cohorts of tools/pileup_bench.py (seeded, written here with
tests/bam_py.write_bam and indexed with tests/bai_py.write_bai), one window, and two routes from BAM files to a pileup in device
memory:

    parent   BamFile::next_raw on T threads (the host reads AND inflates with zlib), then bv_engine_pileup from host records
    members  read_window_members on T threads (the host only reads compressed members: basevar_amd/host/raw_members.hpp), then
             bv_engine_pileup_bgzf, which inflates and piles up on the device

    python3 tools/pileup_bgzf_bench.py --samples 100 --depth 8 --rows 100000 --threads 1 16 [--out profiles/pileup_bgzf_bench.txt]
    python3 tools/pileup_bgzf_bench.py --samples 10000 --depth 0.5 --rows 13000 --threads 1 16 --append

Both reads are timed by tests/cpp/bam_members_check.cpp `time`, three passes each with the readers kept open; the engine calls
are timed here, alternated, four passes each.  Every figure is the best of the passes it prints (the first engine pass
allocates and does not count).  Also: the inflate alone (bv_engine_bgzf_inflate of the same members into device memory), the
member count, and the ratio of the bytes inflated to the bytes the pile kernel walks.  Both routes give the same planes
(tests/test_gpu_pileup_bgzf.py); the bench checks the covered-row count and the depths."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bai_py  # noqa: E402
import bam_members as bm  # noqa: E402
import pileup_ref as pr  # noqa: E402
from pileup_bench import write_cohort  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--depth", type=float, default=8.0)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--no-index", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    import torch
    import basevar_amd as bv
    exe = bm.build()
    beg, end = 1000, 1000 + a.rows - 1
    assert end <= pr.STEP
    lines = ["# tools/pileup_bgzf_bench.py --samples %d --depth %g --rows %d%s (window %d-%d of %s, seed %d)" % (
        a.samples, a.depth, a.rows, " --no-index" if a.no_index else "", beg, end, pr.REF_ID, a.seed)]
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        fasta, fa, bams = write_cohort(d, a.samples, a.depth, beg, end, a.seed)
        if not a.no_index:
            for b in bams:
                bai_py.write_bai(b)
        lines.append("cohort written%s in %.1f s" % ("" if a.no_index else " and indexed", time.perf_counter() - t0))
        runs_path, mem_path = os.path.join(d, "runs.bin"), os.path.join(d, "members.bin")
        read = {}
        for t in a.threads:
            out = subprocess.check_output([exe, "time", runs_path, mem_path, pr.REF_ID, str(beg), str(end), str(t)] + bams).decode()
            lines += ["  " + l for l in out.strip().split("\n")]
            read[t] = (min(float(x) for x in re.findall(r"raw records read ([0-9.]+) s", out)), min(float(x) for x in re.findall(r"members read ([0-9.]+) s", out)))
        tid = int(re.search(r"tid (-?\d+)", out).group(1))
        b = open(runs_path, "rb").read()
        n_runs, n_samples = np.frombuffer(b, "<u4", 2)
        run_off = np.frombuffer(b, "<u8", n_runs + 1, 8).copy()
        run_sample = np.frombuffer(b, "<u4", n_runs, 8 + 8 * (n_runs + 1)).copy()
        records = np.frombuffer(b, np.uint8, offset=8 + 12 * n_runs + 8).copy()
        p = bm.parse_members(mem_path)
    eng = bv.BaseTypeEngine(max_sites=1024, min_af_value=bv.min_af(a.samples), device=0, max_samples=a.samples)
    eng.pileup_set_reference(fa)
    n_members = len(p.member_off) - 1
    dst_off = np.concatenate([[0], np.cumsum(p.isize)]).astype(np.int64)
    r = p.runs
    walked = int(((dst_off[r["first_member"] + r["n_members"] - 1] + r["end"]) - (dst_off[r["first_member"]] + r["begin"])).sum())
    inflated = int(dst_off[-1])
    d_text = torch.empty(max(inflated, 16), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    best = {"parent": 1e9, "members": 1e9, "inflate": 1e9, "rows": 1e9}
    depth = {}
    for rep in range(4):
        t0 = time.perf_counter()
        n_a = eng.pileup(records, run_off, run_sample, a.samples, tid, pr.REGION, (beg, end), pr.MAPQ_THD)
        t1 = time.perf_counter()
        eng.pileup_rows(tagged=True)
        t2 = time.perf_counter()
        if rep == 0:
            depth["parent"] = eng.pileup_fetch()["depth"].tobytes()
        t3 = time.perf_counter()
        n_b = eng.pileup_bgzf(p.data, p.member_off, p.runs, a.samples, tid, pr.REGION, (beg, end), pr.MAPQ_THD)
        t4 = time.perf_counter()
        eng.pileup_rows(tagged=True)
        if rep == 0:
            depth["members"] = eng.pileup_fetch()["depth"].tobytes()
        t5 = time.perf_counter()
        eng.bgzf_inflate(p.data, p.member_off, dst_ptr=int(d_text.data_ptr()), dst_capacity=int(d_text.numel()))
        t6 = time.perf_counter()
        assert n_a == n_b, (n_a, n_b)
        lines.append("  pass %d: bv_engine_pileup (host records) %.6f s, bv_engine_pileup_rows %.6f s; bv_engine_pileup_bgzf %.6f s; "
                     "bv_engine_bgzf_inflate of the same members alone %.6f s; covered %d" % (rep, t1 - t0, t2 - t1, t4 - t3, t6 - t5, n_b))
        if rep:
            best = {"parent": min(best["parent"], t1 - t0), "rows": min(best["rows"], t2 - t1), "members": min(best["members"], t4 - t3), "inflate": min(best["inflate"], t6 - t5)}
    assert depth["parent"] == depth["members"]
    lines.append("summary, %d samples, %d rows, %d covered: %.1f MB of records in %d runs (parent); %d members of %.1f MB in %d runs, inflating to %.1f MB, "
                 "of which the pile kernel walks %.1f MB (inflated / walked = %.2f)" % (
                     a.samples, a.rows, n_b, records.size / 1e6, n_runs, n_members, p.data.size / 1e6, len(r), inflated / 1e6, walked / 1e6, inflated / max(walked, 1)))
    lines.append("  engine calls: bv_engine_pileup (host records) %.4f s; bv_engine_pileup_bgzf %.4f s, the inflate alone %.4f s (%.0f %% of the call, %.2f ms per 500 members)" % (
        best["parent"], best["members"], best["inflate"], 100 * best["inflate"] / best["members"], 1e3 * best["inflate"] * 500 / max(n_members, 1)))
    for t in a.threads:
        raw, mem = read[t]
        pa, me = raw + best["parent"] + best["rows"], mem + best["members"] + best["rows"]
        lines.append("  %2d host thread(s): parent route %.4f s (next_raw %.4f + pileup %.4f + rows %.4f); members route %.4f s (member read %.4f + pileup_bgzf %.4f + "
                     "rows %.4f) = %.2f x" % (t, pa, raw, best["parent"], best["rows"], me, mem, best["members"], best["rows"], pa / me))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
