#!/usr/bin/env python3
"""MB/s of text of bv_engine_bgzf_deflate (host text, host members) beside single-thread zlib on the same host, and the size
of what it writes against zlib's.

    python3 tools/bgzf_deflate_bench.py [--blocks 500 45000] [--repeat 5] [--sizes-only] [--level fast|small]

The text is VCF records as host/vcf_emit.hpp writes them (tests/cpp/emit_corpus.cpp: 10,000 samples at coverage 0.08, about
50 KB a record), cut into blocks of 0xff00 bytes: 48 distinct blocks, repeated.  The engine's figure is the wall time of the
whole call -- the text through the pinned staging, the deflate kernel, the prefix sum and the gather of the members, the
members back -- median of --repeat calls after one warm-up; the kernel's own time is what `rocprofv3 --kernel-trace --stats`
of this script shows for bv_bgzf_deflate_kernel (--level small: bv_bgzf_small_kernel); a call with one block, which is
one wave's latency and what a writer with few blocks a batch waits for, is timed as well.  zlib's figures are zlib.compressobj(level, DEFLATED, -15) over the same
blocks, one thread.  The sizes (whole members, 26 bytes of wrapper each) are given for VCF records, CVG rows and batchfile
rows."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BLOCK = 0xff00


def zlib_bytes(blocks, level):
    total, t0 = 0, time.perf_counter()
    for b in blocks:
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += 26 + len(co.compress(b)) + len(co.flush())
    return total, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, nargs="+", default=[500, 45000])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sizes-only", action="store_true")
    ap.add_argument("--level", choices=["fast", "small"], default="fast")
    a = ap.parse_args()
    import basevar_amd as bv
    import bgzf_corpus as bc
    import deflate_corpus as dc
    eng = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(10000), device=0)
    with tempfile.TemporaryDirectory() as d:
        emit = dc.cxx("emit_corpus", d)
        vcf = dc.emitted(emit, "vcf", 10000, 64, 21)[:48 * BLOCK]
        cvg = dc.emitted(emit, "cvg", 10000, 60000, 22)[:48 * BLOCK]
    rows = b"".join(bc.rows_text(BLOCK, seed=100 + k) for k in range(48))
    assert len(vcf) == len(cvg) == len(rows) == 48 * BLOCK
    for name, text in (("VCF records", vcf), ("CVG rows", cvg), ("batchfile rows", rows)):
        blocks = [text[k:k + BLOCK] for k in range(0, len(text), BLOCK)]
        members, off = eng.bgzf_deflate(text, level=a.level)
        back, _, status = eng.bgzf_inflate(members, off)
        assert not status.any() and back.tobytes() == text
        l1, _ = zlib_bytes(blocks, 1)
        l6, _ = zlib_bytes(blocks, 6)
        print("[%s] %-15s %8d B of text in 48 blocks: device members %8d B (%5.2f x smaller than the text)   zlib level 1 %8d B (device = %.3f x)   level 6 %8d B (device = %.3f x)"
              % (a.level, name, len(text), members.size, len(text) / members.size, l1, members.size / l1, l6, members.size / l6), flush=True)
    if a.sizes_only:
        return
    pool = [vcf[k:k + BLOCK] for k in range(0, len(vcf), BLOCK)]
    z = {}
    for level in (1, 6):
        _, t = zlib_bytes(pool * 4, level)
        z[level] = t / (4 * len(pool))  # seconds a block
    one = []
    for r in range(4 * a.repeat + 1):
        t0 = time.perf_counter()
        eng.bgzf_deflate(pool[r % len(pool)], level=a.level)
        one.append(time.perf_counter() - t0)
    print("[%s] one block of %d B alone: engine call %.2f ms (median of %d; zlib level 1 %.2f ms, level 6 %.2f ms)"
          % (a.level, BLOCK, statistics.median(one[1:]) * 1e3, len(one) - 1, z[1] * 1e3, z[6] * 1e3), flush=True)
    for n in a.blocks:
        text = np.frombuffer(vcf * (n // 48) + vcf[:(n % 48) * BLOCK], np.uint8)
        assert text.size == n * BLOCK
        times = []
        for r in range(a.repeat + 1):
            t0 = time.perf_counter()
            members, off = eng.bgzf_deflate(text, level=a.level)
            times.append(time.perf_counter() - t0)
            assert len(off) == n + 1
        t_gpu = statistics.median(times[1:])
        mb = text.size / 1e6
        print("[%s] %6d blocks  %8.1f MB of VCF text -> %7.1f MB   engine call %9.2f ms  %8.1f MB/s   zlib 1 thread: level 1 %9.1f ms %6.1f MB/s (%5.1f x)   level 6 %9.1f ms %6.1f MB/s (%5.1f x)"
              % (a.level, n, mb, members.size / 1e6, t_gpu * 1e3, mb / t_gpu, z[1] * n * 1e3, mb / (z[1] * n), z[1] * n / t_gpu, z[6] * n * 1e3, mb / (z[6] * n),
                 z[6] * n / t_gpu), flush=True)
        del text, members
    eng.close()


if __name__ == "__main__":
    main()
