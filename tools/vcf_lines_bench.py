#!/usr/bin/env python3
"""Times of bv_engine_vcf_format / _deflate (include/basevar_amd_vcf.h) on the recorded job's VCF output -- 4,800 lines x
10,000 samples at coverage 0.08, about 243 MB of text -- beside the route the lines take without it.

    python3 tools/vcf_lines_bench.py [--lines 4800] [--samples 10000] [--repeat 5] [--device-only]

Device planes in, as bv_engine_text_submit leaves them.  Reported, each the median of --repeat calls after one warm-up, wall
time of the whole blocking call:
  vcf_format                       heads up, count + scan + write kernels, line_off back
  vcf_format + vcf_deflate (fast)  ... and the members back: what `bv_call --emit device` does for a *.vcf.gz
  the route without it             the two planes back to pageable host memory, format_vcf_line on one thread (the harness
                                   tests/cpp/vcf_lines_check.cpp --time), bgzf_deflate of the host text (fast)
and the bytes the write kernel moves (2 B read per cell + the text written): its own time is what `rocprofv3 --kernel-trace
--stats` of this script with --device-only shows for bv_vcf_write_kernel; bytes over that time stands beside the 6.3 TB/s a
streaming kernel achieves on this device.  The device's text is compared with the harness's before anything is reported."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_s(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=4800)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--coverage", type=float, default=0.08)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device-only", action="store_true", help="the engine's calls alone (for a profiler run)")
    a = ap.parse_args()
    import torch
    import basevar_amd as bv
    from basevar_amd import _capi
    import vcf_lines_ref as vr
    L, N = a.lines, a.samples
    rng = np.random.default_rng(7)
    covered = rng.random((L, N)) < a.coverage
    cell = np.where(covered, rng.integers(0, 8, (L, N)), 8).astype(np.uint8)
    phred = np.where(covered, np.clip(rng.normal(32, 6, (L, N)), 2, 41), 0).astype(np.uint8)
    pitch = (N + 15) // 16 * 16
    planes = []
    for p in (cell, phred):
        t = torch.full((L, pitch), 8, dtype=torch.uint8, device="cuda")
        t[:, :N] = torch.from_numpy(p).cuda()
        planes.append(t)
    torch.cuda.synchronize()
    slab = _capi.Slab(L, N, pitch, int(planes[0].data_ptr()), int(planes[1].data_ptr()), None, None, None, None, 0, _capi.BV_MEM_DEVICE, 0, 0)
    # eight seeded records, taken in turn: their heads and gt from the harness, as the tests take them
    exe = vr.build()
    recs = []
    for k in range(8):
        ref = k % 4
        recs.append((vr.record(rng, [(ref + 1 + k // 4) & 3])[0], vr.BASES[ref:ref + 1]))
    lines = [vr.line(k, recs[k % 8][0], ref_base=recs[k % 8][1], ref_pos=10000 + 5 * k, ref_id=b"chr%d" % (1 + 3 * k // (L + 1))) for k in range(L)]
    with tempfile.TemporaryDirectory() as d:
        # (heads hold the position: one harness run over rows of one sample gives every line's head and gt cheaply)
        one = vr.run(exe, cell[:, :1], phred[:, :1], lines, tmp_dir=d)
        heads, gt = [h for h, _, _ in one], np.stack([g for _, g, _ in one])
        eng = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(N), device=0, max_samples=N)
        site = np.arange(L, dtype=np.uint32)
        off = eng.vcf_format(site, heads, gt, slab)
        total = int(off[-1])
        cells = L * N
        print("%d lines x %d samples, coverage %.3f: %d bytes of text (%.1f MB), heads %d bytes" % (L, N, a.coverage, total, total / 1e6, sum(map(len, heads))))
        f = median_s(lambda: eng.vcf_format(site, heads, gt, slab), a.repeat)
        print("vcf_format, whole call:                 median %.2f ms (min %.2f, max %.2f) = %.1f GB/s of text" % (f[0] * 1e3, f[1] * 1e3, f[2] * 1e3, total / f[0] / 1e9))

        def both():
            eng.vcf_format(site, heads, gt, slab)
            return eng.vcf_deflate(level="fast")
        fd = median_s(both, a.repeat)
        members, moff = both()
        print("vcf_format + vcf_deflate (fast):        median %.2f ms (min %.2f, max %.2f); %d members, %d bytes" % (fd[0] * 1e3, fd[1] * 1e3, fd[2] * 1e3, moff.size - 1, members.size))
        print("write kernel bytes: %d read (2 B a cell) + %d written = %d; at 6.3 TB/s: %.3f ms" % (2 * cells, total, 2 * cells + total, (2 * cells + total) / 6.3e12 * 1e3))
        if a.device_only:
            eng.close()
            return
        # the route without it
        fin, fout = os.path.join(d, "all.in"), os.path.join(d, "all.out")
        import struct
        parts = [struct.pack("<4I", L, N, L, 0), cell.tobytes(), phred.tobytes()]
        for ln in lines:
            parts += [struct.pack("<III", ln["site"], ln["ref_pos"], len(ln["ref_id"])), ln["ref_id"], struct.pack("<I", len(ln["ref_base"])), ln["ref_base"],
                      struct.pack("<i", -1), ln["rec"].tobytes()]
        open(fin, "wb").write(b"".join(parts))
        out = subprocess.check_output([exe, fin, fout, "--time"]).decode().split()
        host_format_s, host_bytes = float(out[1]), int(out[3])
        host_text = np.fromfile(fout, dtype=np.uint8)
        dev_text = eng.vcf_fetch()
        assert host_bytes == total and host_text.tobytes() == dev_text.tobytes(), "the device's text is not the host formatter's"
        back = median_s(lambda: (planes[0].cpu(), planes[1].cpu()), a.repeat)
        hd = median_s(lambda: eng.bgzf_deflate(host_text, level="fast"), a.repeat)
        ref_members, _ = eng.bgzf_deflate(host_text, level="fast")
        assert ref_members.tobytes() == members.tobytes()
        print("the device's text and members are the host route's, byte for byte")
        print("the route without it: planes back %.2f ms + format_vcf_line on one thread %.1f ms (%.0f MB/s) + bgzf_deflate from host text %.2f ms = %.1f ms"
              % (back[0] * 1e3, host_format_s * 1e3, total / host_format_s / 1e6, hd[0] * 1e3, (back[0] + host_format_s + hd[0]) * 1e3))
        print("vcf_format + vcf_deflate against it: %.1f x" % ((back[0] + host_format_s + hd[0]) / fd[0]))
        eng.close()


if __name__ == "__main__":
    main()
