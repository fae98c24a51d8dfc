#!/usr/bin/env python3
"""packed_tile_job.py -- BASELINE configs[4]'s tile job from packed host tiles: one bv_engine_tiles_add_sparse per tile against
bv_engine_tiles_add_sparse_many in calls of k tiles, beside the dense host tiles of the same job (the link rate the packed legs
are held to).

    python tools/packed_tile_job.py [--sites 16384] [--samples 1000000] [--tile-width 200] [--jobs 3] [--batches 32,256,0]

The job: --sites sites x --samples samples in tiles of --tile-width samples, cut from a synthetic slab on the device; --distinct
distinct tiles, each ONE pinned allocation first touched on the GPU's NUMA node, cycled over the job (bench.py --tile-job's
TileRig).  The legs run in turn, --jobs rounds of one job each (after one untimed round); every job is begin + tiles + finish +
bv_engine_wait, timed on the host.  The records of every leg must be those of the dense leg, byte for byte.  Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sites", type=int, default=16384)
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--tile-width", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=64, help="distinct host tiles, cycled over the job")
    ap.add_argument("--jobs", type=int, default=3, help="timed jobs per leg (legs alternate)")
    ap.add_argument("--batches", default="32,256,0", help="tiles per bv_engine_tiles_add_sparse_many call, 0 = the whole job")
    ap.add_argument("--coverage", type=float, default=0.08)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense-tile leg")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import basevar_amd
    from basevar_amd import _capi
    from bench import TileRig

    dev = torch.device("cuda", 0)
    St, W = args.sites, args.tile_width
    n_tiles = max(1, args.samples // W)
    res = max(1, min(n_tiles, args.distinct))
    N = n_tiles * W
    N_fill = res * W
    pitch = (N_fill + 255) // 256 * 256
    bs = torch.empty((St, pitch), dtype=torch.uint8, device=dev)
    q = torch.empty_like(bs)
    mq = torch.empty_like(bs)
    rp = torch.empty((St, pitch), dtype=torch.int16, device=dev)
    ref = torch.empty(St, dtype=torch.uint8, device=dev)
    basevar_amd.synth_fill(0, St, N_fill, pitch, bs.data_ptr(), q.data_ptr(), ref.data_ptr(), mq.data_ptr(), rp.data_ptr(),
                           coverage=args.coverage)
    torch.cuda.synchronize()
    eng = basevar_amd.BaseTypeEngine(max_sites=St, min_af_value=basevar_amd.min_af(N), device=0, max_samples=N)
    rig = TileRig(torch, eng, dev, 0, St, W, n_tiles, res, (bs, q, mq, rp, ref), host=not args.no_dense)
    rig.build_packed()
    sparse = rig._sparse
    lib = eng._lib

    def job_many(out_ptr, k):
        rc = lib.bv_engine_tiles_begin(eng._h, St, N, 0, 1)
        assert rc == 0, eng._err()
        k = k or len(sparse)
        for i in range(0, len(sparse), k):
            eng.tiles_add_sparse_many(sparse[i:i + k])
        rc = lib.bv_engine_tiles_finish(eng._h, rig.ref.data_ptr(), out_ptr, None, _capi.BV_MEM_DEVICE, None)
        assert rc == 0, eng._err()

    legs = []
    if not args.no_dense:
        legs.append(("dense_tiles_add", lambda o: rig.job(o, _capi.BV_MEM_HOST), rig.host_bytes_per_job()))
    legs.append(("packed_add_sparse", lambda o: rig.job_packed(o), rig.packed_host_bytes_per_job()))
    for k in (int(x) for x in args.batches.split(",") if x.strip()):
        legs.append(("packed_add_sparse_many_%s" % (k if k else "all"), lambda o, k=k: job_many(o, k), rig.packed_host_bytes_per_job()))
    rec = basevar_amd.SITE_DTYPE.itemsize
    outs = {name: torch.zeros(St * rec, dtype=torch.uint8, device=dev) for name, _, _ in legs}
    times = {name: [] for name, _, _ in legs}
    for rnd in range(args.jobs + 1):  # round 0: untimed (allocations, staging ring, first touch)
        for name, run, _ in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(outs[name].data_ptr())
            eng.wait()
            dt = time.perf_counter() - t0
            if rnd:
                times[name].append(dt)
    torch.cuda.synchronize()
    first = outs[legs[0][0]]
    identical = all(torch.equal(first, o) for o in outs.values())
    res_legs = {}
    for name, _, nbytes in legs:
        t = statistics.median(times[name])
        res_legs[name] = {"ms_per_job": round(t * 1e3, 2), "ms_per_job_all": [round(x * 1e3, 2) for x in times[name]],
                          "sites_per_s": round(St / t, 1), "host_GBps": round(nbytes / t / 1e9, 2), "host_bytes_per_job": int(nbytes)}
    per_tile = res_legs["packed_add_sparse"]
    many = {k: v for k, v in res_legs.items() if k.startswith("packed_add_sparse_many")}
    best = max(many.values(), key=lambda v: v["sites_per_s"]) if many else None
    line = {"tool": "packed_tile_job", "sites": St, "samples": N, "tile_width": W, "tiles_per_job": n_tiles, "distinct_tiles": res,
            "coverage": args.coverage, "jobs_per_leg": args.jobs, "legs": res_legs, "records_identical_across_legs": bool(identical),
            "numa_node_of_gpu": rig.numa_node,
            "best_batched_vs_per_tile_sites_per_s": round(best["sites_per_s"] / per_tile["sites_per_s"], 3) if best else None,
            "best_batched_GBps_vs_dense_GBps": (round(best["host_GBps"] / res_legs["dense_tiles_add"]["host_GBps"], 3)
                                                if best and "dense_tiles_add" in res_legs else None)}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")
    del outs, rig
    eng.close()
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
