#!/usr/bin/env python3
"""What does parsing a window of batchfile rows a few files at a time cost beside parsing it whole?  Whole blocking calls, wall
time, through the C ABI (include/basevar_amd_text_job.h).

    python3 tools/text_job_bench.py [--positions 240] [--out profiles/text_job_bench.txt] [--once]

The recorded job's shape (tools/text_tokens_bench.py): 240 positions x 10,000 samples in 50 files of 200, rows written from a
seeded slab with 5 % of the covered calls an indel token.  bv_engine_text_parse on the joined rows against
bv_engine_text_job_begin + adds of 1, 8 and 50 files + bv_engine_text_job_finish, with the token mode off and on.  Every figure
is the best and the worst of 5 passes after the first, which allocates.  --once runs every form once and times nothing: the run
to collect kernel times from (rocprofv3 --kernel-trace --stats -- python3 tools/text_job_bench.py --once)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--positions", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import basevar_amd as bv
    from basevar_amd import _capi
    from basevar_amd.synth import make_slab
    from test_gpu_text_rows import slab_rows
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    F, per, P = 50, 200, a.positions
    N, fs = F * per, np.full(F, per, np.uint32)
    slab = make_slab(P, N, seed=5, coverage=0.3, indel_frac=0.05)
    text, off = slab_rows(slab, fs)
    raw = text.tobytes()
    eng = bv.BaseTypeEngine(max_sites=P, min_af_value=bv.min_af(N), device=0, max_samples=N)
    tr = _capi.TextRows(text.ctypes.data, off.ctypes.data, fs.ctypes.data, int(text.size), P, F, 0)
    state = np.zeros((P, F), np.uint8)

    def whole():
        assert eng._lib.bv_engine_text_parse(eng._h, C.byref(tr), None, 0, state.ctypes.data, None) == 0, eng._err()

    def adds_of(K):
        """the rows of every group of K files, packed as an add brings them (kept alive by the list)"""
        out = []
        for first in range(0, F, K):
            k = min(K, F - first)
            flat = [raw[int(off[p * F + first + j]):int(off[p * F + first + j + 1])] for p in range(P) for j in range(k)]
            o = np.zeros(len(flat) + 1, np.uint64)
            o[1:] = np.cumsum([len(r) for r in flat])
            t = np.frombuffer(b"".join(flat), np.uint8)
            out.append((first, _capi.TextRows(t.ctypes.data, o.ctypes.data, fs[first:].ctypes.data, int(t.size), P, k, 0), t, o))
        return out

    def job(adds):
        def run():
            assert eng._lib.bv_engine_text_job_begin(eng._h, P, F, fs.ctypes.data, None, 0, None) == 0, eng._err()
            for first, rows, _, _ in adds:
                assert eng._lib.bv_engine_text_job_add(eng._h, C.byref(rows), first, None, None) == 0, eng._err()
            assert eng._lib.bv_engine_text_job_finish(eng._h, state.ctypes.data, None) == 0, eng._err()
        return run

    groups = {K: adds_of(K) for K in (1, 8, 50)}
    ms = lambda t: "%.3f / %.3f ms" % (1e3 * t[0], 1e3 * t[1])  # noqa: E731
    say("# tools/text_job_bench.py: %d positions x %d samples in %d files, %.1f MB of rows; whole blocking calls, best / worst of 5 passes" % (P, N, F, text.size / 1e6))
    for on in (False, True):
        eng.text_tokens_enable(on)
        if a.once:
            whole()
            ref = state.copy()
            for K in (1, 8, 50):
                job(groups[K])()
                assert np.array_equal(state, ref)
            continue
        t_whole = best_of(whole)
        ref = state.copy()
        say("  token mode %s" % ("on" if on else "off"))
        say("    bv_engine_text_parse, all %d files at once          %s" % (F, ms(t_whole)))
        for K in (1, 8, 50):
            t = best_of(job(groups[K]))
            assert np.array_equal(state, ref)
            say("    job: begin + %2d add(s) of %2d file(s) + finish        %s   (%.2f x the whole parse's best)" % (len(groups[K]), K, ms(t), t[0] / t_whole[0]))
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
