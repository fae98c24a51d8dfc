#!/usr/bin/env python3
"""What does the device's indel tally cost, and how long does its slowest row hold a launch?  Whole blocking calls, wall time.

    python3 tools/indel_tally_bench.py [--samples 10000 --depth 0.5 --rows 13000] [--out profiles/indel_tally_bench.txt]

  (a) the pileup of tools/pileup_bench.py's cohort: bv_engine_indel_tally with tok == NULL over every covered position,
      against the token fetch (descriptors and text, bv_engine_pileup_fetch) plus indel_string over the same tokens on one host
      thread (tests/cpp/indel_tally_check.cpp `time`: the strings made per row, as bv_call made them)
  (b) one row of bv_indel_row_tokens_max() tokens in 8 classes, from host and from device tokens
  (c) one row of 300 distinct tokens
Every figure is the best of the passes after the first, which allocates."""
import argparse
import ctypes as C
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
import indel_tally_ref as ref  # noqa: E402
import pileup_ref as pr  # noqa: E402
from pileup_bench import write_cohort  # noqa: E402


def best_of(fn, passes=5):
    fn()
    out = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--depth", type=float, default=0.5)
    ap.add_argument("--rows", type=int, default=13000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import basevar_amd as bv
    from basevar_amd import _capi
    check = ref.build()
    beg, end = 1000, 1000 + a.rows - 1
    lines = ["# tools/indel_tally_bench.py --samples %d --depth %g --rows %d (window %d-%d of %s, seed %d); wall time of whole blocking calls, best (.. worst) of 5" % (
        a.samples, a.depth, a.rows, beg, end, pr.REF_ID, a.seed)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = bv.BaseTypeEngine(max_sites=1024, min_af_value=bv.min_af(a.samples), device=0, max_samples=a.samples)
    with tempfile.TemporaryDirectory() as d:
        fasta, fa, bams = write_cohort(d, a.samples, a.depth, beg, end, a.seed)
        runs_path = os.path.join(d, "runs.bin")
        out = subprocess.check_output([pr.build(), "time", runs_path, fasta, pr.REF_ID, str(pr.REGION[0]), str(pr.REGION[1]), str(beg), str(end), str(pr.MAPQ_THD), "16"] + bams).decode()
        tid = int(re.search(r"tid (-?\d+)", out).group(1))
        b = open(runs_path, "rb").read()
        n_runs, n_samples = np.frombuffer(b, "<u4", 2)
        run_off = np.frombuffer(b, "<u8", n_runs + 1, 8).copy()
        run_sample = np.frombuffer(b, "<u4", n_runs, 8 + 8 * (n_runs + 1)).copy()
        records = np.frombuffer(b, np.uint8, offset=8 + 12 * n_runs + 8).copy()
        eng.pileup_set_reference(fa)
        n_cov = eng.pileup(records, run_off, run_sample, a.samples, tid, pr.REGION, (beg, end), pr.MAPQ_THD)
        _, pos, _ = eng.pileup_rows(tagged=False)
        res = _capi.PileupResult()
        res.mem_kind = _capi.BV_MEM_HOST
        eng._lib.bv_engine_pileup_fetch(eng._h, C.byref(res), None)
        tokens, text = np.zeros(int(res.n_tokens), _capi.PILEUP_TOKEN_DTYPE), np.zeros(int(res.text_bytes), np.uint8)

        def fetch():
            r = _capi.PileupResult()
            r.mem_kind = _capi.BV_MEM_HOST
            r.tokens, r.text, r.tokens_capacity, r.text_capacity = tokens.ctypes.data, text.ctypes.data, tokens.size, text.size
            assert eng._lib.bv_engine_pileup_fetch(eng._h, C.byref(r), None) == 0
        got = {}

        def tally():
            got["off"], got["flag"] = eng.indel_tally(pos)
        t_fetch, t_tally = best_of(fetch), best_of(tally)
        fin = os.path.join(d, "tally.in")
        rows = ref.Rows([], pos)
        rows.tokens, rows.text = tokens, text  # (as the engine handed them out)
        ref.write_input(fin, rows)
        host = subprocess.check_output([check, "time", fin]).decode().strip()
        t_host = float(re.search(r"time: ([0-9.]+) s", host).group(1))
        n_col = int((np.diff(got["off"]) > 0).sum())
        longest = int(np.bincount(tokens["pos"] - beg).max()) if tokens.size else 0
        say("(a) %d samples, %d covered rows, %d tokens of %d bytes, %d rows with a column (%d bytes), %d flagged, the longest row %d tokens" % (
            a.samples, n_cov, tokens.size, text.size, n_col, int(got["off"][-1]), int(got["flag"].sum()), longest))
        say("  device  indel_tally(tok = NULL), all covered rows          %.6f s (.. %.6f)" % t_tally)
        say("  host    token fetch (descriptors + text)                   %.6f s (.. %.6f)" % t_fetch)
        say("  host    strings + indel_string, one thread                 %.6f s   [%s]" % (t_host, host))
        say("  host    fetch + indel_string                               %.6f s = %.2f x the device's call" % (t_fetch[0] + t_host, (t_fetch[0] + t_host) / t_tally[0]))
    limit = eng.indel_row_tokens_max()
    for title, toks in (("(b) one row of %d tokens in 8 classes" % limit, ref.cycle([ref.distinct(i, 2) for i in range(8)], limit)),
                        ("(c) one row of 300 distinct tokens", [ref.distinct(i) for i in range(300)])):
        rows = ref.Rows([(7, toks)], [7])
        tt = torch.from_numpy(np.frombuffer(rows.tokens.tobytes(), np.uint8).copy()).cuda()
        tx = torch.from_numpy(rows.text.copy()).cuda()
        torch.cuda.synchronize()
        t_host = best_of(lambda: eng.indel_tally(rows.keys, rows.tokens, rows.text))
        t_dev = best_of(lambda: eng.indel_tally(rows.keys, (int(tt.data_ptr()), len(rows.tokens)), (int(tx.data_ptr()), rows.text.size)))
        off, flag = eng.indel_tally(rows.keys, rows.tokens, rows.text)
        assert eng.indel_fetch().tobytes() == rows.expected()[0][1] and not flag.any()
        say("%s (a column of %d bytes)" % (title, int(off[-1])))
        say("  device  indel_tally, host tokens (uploaded)                %.6f s (.. %.6f)" % t_host)
        say("  device  indel_tally, device tokens (checked on the device)  %.6f s (.. %.6f)" % t_dev)
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
