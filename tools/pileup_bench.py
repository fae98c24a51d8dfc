#!/usr/bin/env python3
"""What does the device pileup gain?  A seeded synthetic cohort of BAM files (tests/bam_py.write_bam; nothing but this
repository is needed), one window, and the two routes from reads to slab rows in device memory:

    host     BamFile::next + pileup_tile on T threads, the covered rows copied into a slab, the slab copied up
             (tests/cpp/pileup_core_check.cpp `time`; the copy up is timed here, from pinned memory)
    device   BamFile::next_raw on T threads (the same harness), then bv_engine_pileup + bv_engine_pileup_rows, host records
             (staging included) and device-resident records

    python3 tools/pileup_bench.py --samples 100 --depth 8 --rows 100000 --threads 1 16 [--out profiles/pileup_device_bench.txt]
    python3 tools/pileup_bench.py --samples 10000 --depth 0.5 --rows 13000 --threads 1 16 --append

Every figure is the best of the passes it prints.  Both routes give the same planes (tests/test_gpu_pileup.py); the bench
checks the covered-row count only."""
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
import bam_py  # noqa: E402
import pileup_ref as pr  # noqa: E402

READ_LEN = 150


def write_cohort(directory, n, depth, beg, end, seed):
    """n coordinate-sorted BAMs of 150-base reads at `depth` x over [beg, end] (one read in eight soft-clipped with an insertion
    behind the clip, one in eight with a skip and a deletion), and the FASTA"""
    fa = pr.reference()
    fasta = os.path.join(directory, "ref.fa")
    pr.write_fasta(fasta, fa)
    paths = []
    n_reads = max(1, int(round(depth * (end - beg + 1 + READ_LEN) / READ_LEN)))
    for s in range(n):
        rng = np.random.default_rng(seed + s)
        recs = []
        for pos in sorted(int(x) for x in rng.integers(max(beg - READ_LEN, 1), end, n_reads)):
            k = int(rng.integers(0, 8))
            cigar = [(pr.S, 5), (pr.I, 3), (pr.M, READ_LEN - 8)] if k == 0 else [(pr.M, 70), (pr.N, 20), (pr.D, 2), (pr.M, READ_LEN - 70)] if k == 1 else [(pr.M, READ_LEN)]
            recs.append(pr.read(rng, pos, cigar, mapq=int(rng.choice([5, 30, 60])), flag=16 if rng.random() < 0.5 else 0))
        path = os.path.join(directory, "s%05d.bam" % s)
        bam_py.write_bam(path, pr.REFS, recs)
        paths.append(path)
    return fasta, fa, paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--depth", type=float, default=8.0)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    import torch
    import basevar_amd as bv
    from basevar_amd import _capi
    exe = pr.build()
    beg, end = 1000, 1000 + a.rows - 1
    assert end <= pr.STEP
    lines = ["# tools/pileup_bench.py --samples %d --depth %g --rows %d (reads of %d bases, window %d-%d of %s, seed %d)" % (
        a.samples, a.depth, a.rows, READ_LEN, beg, end, pr.REF_ID, a.seed)]
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        fasta, fa, bams = write_cohort(d, a.samples, a.depth, beg, end, a.seed)
        lines.append("cohort written in %.1f s" % (time.perf_counter() - t0))
        runs_path = os.path.join(d, "runs.bin")
        host = {}
        for t in a.threads:
            out = subprocess.check_output([exe, "time", runs_path, fasta, pr.REF_ID, str(pr.REGION[0]), str(pr.REGION[1]), str(beg), str(end), str(pr.MAPQ_THD), str(t)] + bams).decode()
            lines += ["  " + l for l in out.strip().split("\n")]
            pile = min(float(x) for x in re.findall(r"pileup_tile ([0-9.]+) s", out))
            pack = min(float(x) for x in re.findall(r"rows packed ([0-9.]+) s", out))
            raw = min(float(x) for x in re.findall(r"raw records read ([0-9.]+) s", out))
            covered, pitch = (int(x) for x in re.search(r"covered (\d+), pitch (\d+)", out).groups())
            host[t] = (pile, pack, raw)
        tid = int(re.search(r"tid (-?\d+)", out).group(1))
        b = open(runs_path, "rb").read()
        n_runs, n_samples = np.frombuffer(b, "<u4", 2)
        run_off = np.frombuffer(b, "<u8", n_runs + 1, 8).copy()
        run_sample = np.frombuffer(b, "<u4", n_runs, 8 + 8 * (n_runs + 1)).copy()
        records = np.frombuffer(b, np.uint8, offset=8 + 12 * n_runs + 8).copy()
    eng = bv.BaseTypeEngine(max_sites=1024, min_af_value=bv.min_af(a.samples), device=0, max_samples=a.samples)
    eng.pileup_set_reference(fa)
    d_rec = torch.from_numpy(records).cuda()
    torch.cuda.synchronize()
    dev = {}
    for name, rec in (("host records", records), ("device records", d_rec)):
        best = [1e9, 1e9]
        for rep in range(4):
            t0 = time.perf_counter()
            n_cov = eng.pileup(rec, run_off, run_sample, a.samples, tid, pr.REGION, (beg, end), pr.MAPQ_THD)
            t1 = time.perf_counter()
            eng.pileup_rows(tagged=True)
            t2 = time.perf_counter()
            lines.append("  device, %s, pass %d: bv_engine_pileup %.6f s, bv_engine_pileup_rows %.6f s, covered %d" % (name, rep, t1 - t0, t2 - t1, n_cov))
            if rep:  # (the first pass allocates)
                best = [min(best[0], t1 - t0), min(best[1], t2 - t1)]
        assert n_cov == covered, (n_cov, covered)
        dev[name] = best
    # the copy up of the host route's slab: 5 bytes a cell of the covered rows, from pinned memory
    slab = torch.empty(5 * covered * pitch, dtype=torch.uint8).pin_memory()
    up = 1e9
    for rep in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        slab.cuda(non_blocking=False)
        torch.cuda.synchronize()
        up = min(up, time.perf_counter() - t0)
    lines.append("  copy up of the host slab (%d rows x pitch %d x 5 B = %.1f MB, pinned): %.6f s" % (covered, pitch, 5e-6 * covered * pitch, up))
    lines.append("summary, %d samples, %d rows, %d covered, %.1f MB of records:" % (a.samples, a.rows, covered, records.size / 1e6))
    for t in a.threads:
        pile, pack, raw = host[t]
        h = pile + pack + up
        dh, dd = raw + sum(dev["host records"]), sum(dev["device records"])
        lines.append("  %2d host thread(s): host route %.4f s (pileup_tile %.4f + rows packed %.4f + copy up %.4f); device route %.4f s (raw read %.4f + "
                     "pileup %.4f + rows %.4f) = %.2f x; the engine calls alone on device-resident records %.4f s" % (
                         t, h, pile, pack, up, dh, raw, dev["host records"][0], dev["host records"][1], h / dh, dd))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
