"""Times bv_engine_pileup_text at the two shapes of tools/pileup_bench.py -- 100 samples x 100,000 rows and 10,000 x 13,000, coverage
0.08 -- and writes profiles/pileup_text_bench.txt:
  * pileup_text alone over an explicit tile whose planes lie in device memory (ms, GB/s of text written; the call packs the tile's
    rows with device copies and counts its depths first, which the route from a completed bv_engine_pileup does not need),
  * pileup_text + pileup_text_deflate at both levels, members to host memory,
  * the same shape's text by host/pileup.hpp's pileup_rows_text + BgzfWriter on one host thread (tests/cpp/pileup_text_check.cpp,
    `time` mode, built without sanitizers).
Whole calls, wall clock around a synchronised device; best and median of --repeat runs.

    python tools/pileup_text_bench.py [--repeat 5] [--no-host] [--out profiles/pileup_text_bench.txt]

--parts times, instead, the rows over sample parts at 10,000 samples x 13,000 rows in one sitting, alternated --repeat times:
pileup_text of the whole tile, pileup_text_parts with 50 parts of 200 samples, and 50 pileup_text calls on explicit 200-sample
tiles (the planes' column slices, copied once beforehand); the lines are appended to --parts-out (profiles/pileup_batches_bench.txt).
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(100, 100000), (10000, 13000)]
COVERAGE = 0.08


def planes(n, rows, seed=1):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    pitch = (n + 15) // 16 * 16
    shape = (rows, pitch)
    claimed = torch.rand(shape, generator=g, device="cuda") < COVERAGE
    claimed[:, n:] = False
    cell = torch.randint(0, 8, shape, generator=g, device="cuda", dtype=torch.uint8)
    qual = torch.randint(2, 42, shape, generator=g, device="cuda", dtype=torch.uint8)
    mapq = torch.randint(0, 61, shape, generator=g, device="cuda", dtype=torch.uint8)
    rank = (torch.randint(1, 151, shape, generator=g, device="cuda", dtype=torch.int32) * claimed).to(torch.uint16)
    torch.cuda.synchronize()
    return dict(cell=cell, qual=qual, mapq=mapq, rank=rank, beg=1, n_samples=n)


def timed(fn, repeat):
    import torch
    ts = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts))


def parts_bench(a):
    import basevar_amd as bv
    import pileup_text_parts_model as ppm
    import torch
    n, rows, b = 10000, 13000, 200
    eng = bv.BaseTypeEngine(max_sites=64, min_af_value=0.01, device=0, max_samples=16)
    eng.pileup_set_reference(b"A" * (rows + 1))
    tile = planes(n, rows)
    part_first = list(range(0, n + 1, b))
    pitch_b = (b + 15) // 16 * 16
    slices = []
    for s0 in part_first[:-1]:
        sl = {k: torch.zeros((rows, pitch_b), dtype=tile[k].dtype, device="cuda") for k in ("cell", "qual", "mapq", "rank")}
        for k in sl:
            sl[k][:, :b] = tile[k][:, s0:s0 + b]
        slices.append(dict(sl, beg=1, n_samples=b))
    torch.cuda.synchronize()
    legs = {"pileup_text, the whole tile": lambda: eng.pileup_text("chr1", tile=tile),
            "pileup_text_parts, 50 parts of 200": lambda: eng.pileup_text_parts("chr1", part_first, tile=tile),
            "50 pileup_text calls, 200-sample tiles": lambda: [eng.pileup_text("chr1", tile=sl) for sl in slices]}
    # the timed parts text is the defined one: the last two rows of the last two parts against the serial restatement
    off = eng.pileup_text_parts("chr1", part_first[-3:], rows - 2, 2, tile=tile)
    got = eng.pileup_text_fetch().tobytes()
    import pileup_text_model as ptm
    last = ptm.Tile(b"chr1", rows - 1, n, *[tile[k][rows - 2:].cpu().numpy() for k in ("cell", "qual", "mapq", "rank")], {}, b"A" * (rows + 1))
    assert got == ppm.parts_text(last, part_first[-3:])[0] and int(off[-1]) == len(got), "the device text is not the model's"
    size = int(eng.pileup_text_parts("chr1", part_first, tile=tile)[-1])
    for fn in legs.values():
        fn()  # (the first calls allocate)
    times = {k: [] for k in legs}
    for _ in range(a.repeat):  # alternated
        for k, fn in legs.items():
            times[k].append(timed(fn, 1)[0])
    lines = ["pileup_text_bench --parts: %d samples x %d rows, coverage %.2f, explicit device tiles, %d alternated runs a leg" % (n, rows, COVERAGE, a.repeat),
             "  (each call packs its tile's rows with device copies first, as pileup_text_bench.txt's legs do; parts text %d bytes)" % size]
    for k, ts in times.items():
        lines.append("  %-40s best %9.2f  median %9.2f ms   runs: %s" % (k, min(ts), float(np.median(ts)), " ".join("%.2f" % t for t in ts)))
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.parts_out), exist_ok=True)
    with open(a.parts_out, "a") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup_text_bench.txt"))
    ap.add_argument("--parts", action="store_true")
    ap.add_argument("--parts-out", default=os.path.join(ROOT, "profiles", "pileup_batches_bench.txt"))
    a = ap.parse_args()
    if a.parts:
        return parts_bench(a)
    import basevar_amd as bv
    import pileup_text_model as ptm
    lines = ["pileup_text_bench: coverage %.2f, explicit device tiles, %d runs a leg (best / median ms)" % (COVERAGE, a.repeat)]
    eng = bv.BaseTypeEngine(max_sites=64, min_af_value=0.01, device=0, max_samples=16)
    for n, rows in SHAPES:
        eng.pileup_set_reference(b"A" * (rows + 1))
        tile = planes(n, rows)
        off = eng.pileup_text("chr1", tile=tile)  # (the first call allocates)
        size = int(off[-1])
        best, med = timed(lambda: eng.pileup_text("chr1", tile=tile), a.repeat)
        # the timed text is the defined one: its last two rows against the serial restatement
        part_off = eng.pileup_text("chr1", rows - 2, 2, tile=tile)
        part = eng.pileup_text_fetch().tobytes()
        last = ptm.Tile(b"chr1", rows - 1, n, *[tile[k][rows - 2:].cpu().numpy() for k in ("cell", "qual", "mapq", "rank")], {}, b"A" * (rows + 1))
        assert part == ptm.rows_text(last)[0] and int(part_off[-1]) == int(off[-1] - off[-3]), "the device text is not the model's"
        lines.append("%d samples x %d rows: text %d bytes" % (n, rows, size))
        lines.append("  pileup_text                         %9.2f / %9.2f ms  = %.1f GB/s of text" % (best, med, size / best / 1e6))
        for level in ("fast", "small"):
            eng.pileup_text_deflate(level=level)
            best, med = timed(lambda: (eng.pileup_text("chr1", tile=tile), eng.pileup_text_deflate(level=level)), max(2, a.repeat // 2))
            members = eng.pileup_text_deflate(level=level)[0]
            lines.append("  pileup_text + pileup_text_deflate %-5s %9.2f / %9.2f ms  members %d bytes" % (level, best, med, members.size))
            del members
        if not a.no_host:
            exe = ptm.build(asan=False)
            out = subprocess.run([exe, "time", str(n), str(rows), str(int(COVERAGE * 100))], capture_output=True, text=True, check=True).stdout.strip()
            lines.append("  one host thread: " + out)
        del tile
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
