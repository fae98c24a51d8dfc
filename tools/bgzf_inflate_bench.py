#!/usr/bin/env python3
"""GB/s of inflated text of bv_engine_bgzf_inflate (device destination) beside single-thread zlib on the same host.

    python3 tools/bgzf_inflate_bench.py [--members 500 45000] [--level 1 6] [--repeat 5]

The members are batchfile rows in the reference's format (200 samples per file, coverage 0.08), 0xff00 bytes of text each,
deflated by zlib at the given level: 48 distinct members, repeated.  The engine's figure is the wall time of the whole call --
the compressed bytes through the pinned staging, the inflate kernel, the statuses back -- median of --repeat calls after one
warm-up; the kernel's own time is what `rocprofv3 --kernel-trace --stats` of this script shows for bv_bgzf_inflate_kernel.
zlib's figure is zlib.decompress over the same members, one thread."""
import argparse
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[500, 45000])
    ap.add_argument("--level", type=int, nargs="+", default=[1, 6])
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import torch
    import basevar_amd as bv
    import bgzf_corpus as bc
    eng = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(10000), device=0)
    texts = [bc.rows_text(0xff00, seed=100 + k) for k in range(48)]
    for level in a.level:
        pool = [bc.member(t, level) for t in texts]
        ratio = sum(len(t) for t in texts) / sum(len(m) for m in pool)
        for n in a.members:
            members = [pool[k % len(pool)] for k in range(n)]
            data = np.frombuffer(b"".join(members), np.uint8)
            off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.uint64)
            total = sum(len(texts[k % len(pool)]) for k in range(n))
            dst = torch.empty(total, dtype=torch.uint8, device="cuda:0")
            times = []
            for r in range(a.repeat + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, dst_off, status = eng.bgzf_inflate(data, off, dst_ptr=dst.data_ptr(), dst_capacity=total)
                times.append(time.perf_counter() - t0)
                assert int(dst_off[-1]) == total and not status.any()
            head = bytes(dst[:len(texts[0])].cpu().numpy())
            assert head == texts[0]
            t_gpu = statistics.median(times[1:])
            k = min(n, 2000)  # zlib: enough members for a steady figure
            t0 = time.perf_counter()
            for m in members[:k]:
                zlib.decompress(m[18:-8], -15)
            t_z = (time.perf_counter() - t0) * n / k
            print("level %d  %6d members  %8.1f MB text (%.1f x compressed)   engine call %8.2f ms  %6.2f GB/s   zlib 1 thread %9.1f ms  %5.2f GB/s   %5.1f x"
                  % (level, n, total / 1e6, ratio, t_gpu * 1e3, total / t_gpu / 1e9, t_z * 1e3, total / t_z / 1e9, t_z / t_gpu), flush=True)
            del dst
    eng.close()


if __name__ == "__main__":
    main()
