#!/usr/bin/env python3
"""Times of bv_engine_cvg_format and bv_engine_vcf_format_records + bv_engine_vcf_deflate (include/basevar_amd_record_text.h)
beside the host formatters, on seeded records: about 72,000 records at 100 samples (the BAM route's ground: the heads and the
CVG rows dominate) and about 4,800 records at 10,000 samples (the sample columns dominate).

    python3 tools/record_text_bench.py [--repeat 5] [--out profiles/record_text_bench.txt]

Each figure is the median (min .. max) of --repeat blocking calls after one warm-up, wall time of the whole call, records and
planes in device memory.  The host leg is one thread: format_vcf_head and format_cvg_line inside the stand-alone harness
(tests/cpp/record_text_check.cpp: its whole run, reading and writing its files included, so an upper bound), then vcf_format +
vcf_deflate given those heads.  The device's texts are compared with the harness's before anything is reported."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return "%.4f s (%.4f .. %.4f)" % (statistics.median(ts), min(ts), max(ts))


def main():
    import torch
    import basevar_amd as bv
    from basevar_amd import _capi
    import record_text_model as model
    import record_text_ref as ref
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    exe = ref.build()
    out = ["# tools/record_text_bench.py --repeat %d; seeded records, two pop-groups, coverage 0.08; wall time of whole blocking calls" % a.repeat]
    for n_lines, n_samples in ((72000, 100), (4800, 10000)):
        rng = np.random.default_rng(n_samples)
        names = [b"pop0", b"pop1"]
        lines = []
        for k in range(n_lines):
            alts = [int(x) for x in rng.permutation(4)[:1 + k % 2]]
            r, g = ref.record(rng, alts, 2)
            lines.append(ref.line(r, g, chrom=b"chr1", pos=1000 + k, ref=b"ACGT"[k % 4:k % 4 + 1], tokens=[b"+AT"] if k % 200 == 0 else ()))
        sites = np.array([ln["rec"] for ln in lines], dtype=_capi.SITE_DTYPE)
        groups = np.array([ln["groups"] for ln in lines], dtype=_capi.GROUP_DTYPE)
        pos = np.array([ln["pos"] for ln in lines], np.uint32)
        refs = b"".join(ln["ref"] for ln in lines)
        n_rows = 256
        pitch = (n_samples + 15) // 16 * 16
        cell = np.where(rng.random((n_rows, pitch)) < 0.08, rng.integers(0, 8, (n_rows, pitch)), 8).astype(np.uint8)
        phred = rng.integers(2, 42, (n_rows, pitch)).astype(np.uint8)
        d_cell, d_phred = torch.from_numpy(cell).cuda(), torch.from_numpy(phred).cuda()
        d_sites = torch.from_numpy(np.frombuffer(sites.tobytes(), np.uint8).copy()).cuda()
        d_groups = torch.from_numpy(np.frombuffer(groups.tobytes(), np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        slab = _capi.Slab(n_rows, n_samples, pitch, int(d_cell.data_ptr()), int(d_phred.data_ptr()), None, None, None, None, 0, _capi.BV_MEM_DEVICE, 0, 0)
        site = (np.arange(n_lines) % n_rows).astype(np.uint32)
        rec, grp = (int(d_sites.data_ptr()), n_lines), (int(d_groups.data_ptr()), 2)
        eng = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(n_samples), device=0, max_samples=n_samples)
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            dump = ref.run_lines(exe, lines, names, d)
            host_format = time.perf_counter() - t0
        indel = [None if x[4] == b"." else x[4] for x in dump]
        heads = [x[2] for x in dump]
        gt = np.array([list(model.gt_codes(ln["rec"], ln["ref"])) for ln in lines], np.uint8)
        off = eng.cvg_format(rec, b"chr1", pos, refs, indel=indel, groups=grp, group_names=names)
        assert eng.cvg_fetch().tobytes() == b"".join(x[3] for x in dump)
        cvg_bytes = int(off[-1])
        off = eng.vcf_format_records(site, rec, b"chr1", pos, refs, groups=grp, group_names=names, slab=slab)
        text = eng.vcf_fetch().tobytes()
        eng.vcf_format(site, heads, gt, slab)
        assert text == eng.vcf_fetch().tobytes()
        out.append("%d records x %d samples: CVG text %.1f MB, heads %.1f MB, VCF text %.1f MB" % (n_lines, n_samples, cvg_bytes / 1e6, sum(map(len, heads)) / 1e6, len(text) / 1e6))
        out.append("  device  cvg_format                                   %s" % timed(lambda: eng.cvg_format(rec, b"chr1", pos, refs, indel=indel, groups=grp, group_names=names), a.repeat))
        out.append("  device  cvg_format + cvg_fetch                       %s" % timed(lambda: (eng.cvg_format(rec, b"chr1", pos, refs, indel=indel, groups=grp, group_names=names), eng.cvg_fetch()), a.repeat))
        out.append("  device  vcf_format_records                           %s" % timed(lambda: eng.vcf_format_records(site, rec, b"chr1", pos, refs, groups=grp, group_names=names, slab=slab), a.repeat))
        out.append("  device  vcf_format_records + vcf_deflate (fast)      %s" % timed(lambda: (eng.vcf_format_records(site, rec, b"chr1", pos, refs, groups=grp, group_names=names, slab=slab), eng.vcf_deflate()), a.repeat))
        out.append("  host    format_vcf_head + format_cvg_line (harness)  %.4f s (one run, one thread, file traffic included)" % host_format)
        out.append("  host heads, then vcf_format + vcf_deflate (fast)     %s" % timed(lambda: (eng.vcf_format(site, heads, gt, slab), eng.vcf_deflate()), a.repeat))
        eng.close()
        print("\n".join(out[-7:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
