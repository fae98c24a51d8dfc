"""bench.py --dump-outputs: what the timed path computed in its last step, as float64 .npy files, at most 64 MB in all,
the same for the same arguments (so that two builds can be compared output for output)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from basevar_amd._capi import GROUP_DTYPE, SITE_DTYPE  # noqa: E402


def _records(S, G, seed):
    rng = np.random.default_rng(seed)
    recs = np.frombuffer(rng.integers(0, 256, S * SITE_DTYPE.itemsize, dtype=np.uint8).tobytes(), dtype=SITE_DTYPE)
    grecs = np.frombuffer(rng.integers(0, 256, S * G * GROUP_DTYPE.itemsize, dtype=np.uint8).tobytes(),
                          dtype=GROUP_DTYPE).reshape(S, G) if G else None
    recs = recs.copy()
    for k, x in enumerate((np.nan, np.inf, -np.inf)):  # what the records hold where a value is undefined, and the infinities
        recs["qual"][k::7] = x
        recs["af"][k::5, k] = x
        if G:
            grecs = grecs.copy()
            grecs["af"][k::3, :, k] = x
    return recs, grecs


def _load(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, "*.npy")))}


def _restored(got, name):
    """the record's values of `name` again: the finite values, NaN / +inf / -inf where <name>_nonfinite says so"""
    v = got[name].copy()
    if name + "_nonfinite" in got:
        c = got[name + "_nonfinite"]
        assert c.dtype == np.float32 and c.shape == v.shape and (v[c != 0] == 0).all()
        v[c == 1], v[c == 2], v[c == 3] = np.nan, np.inf, -np.inf
    return v


def _floats(dtype, prefix=""):
    return {prefix + n + "_nonfinite" for n in dtype.names if dtype[n].base.kind == "f"}


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("S,G", [(1000, 0), (300, 3)])
def test_dump_writes_every_field_of_every_site(tmp_path, S, G):
    recs, grecs = _records(S, G, 1)
    assert bench.dump_outputs(str(tmp_path), recs, grecs, 7) == S
    got = _load(str(tmp_path))
    want = set(SITE_DTYPE.names) | {"site_index"} | _floats(SITE_DTYPE)
    if G:
        want |= {"group_" + n for n in GROUP_DTYPE.names if not n.startswith("reserved")} | _floats(GROUP_DTYPE, "group_")
    assert set(got) == want
    assert all(np.isfinite(v).all() for v in got.values())
    assert np.array_equal(got["site_index"], np.arange(S))
    assert {0, 1, 2, 3} <= set(np.unique(got["qual_nonfinite"]).tolist())
    for n in SITE_DTYPE.names:
        assert got[n].dtype == np.float64 and got[n].shape == (S,) + SITE_DTYPE[n].shape
        assert np.array_equal(_restored(got, n), recs[n].astype(np.float64), equal_nan=True), n
    if G:
        assert got["group_af"].shape == (S, G, 4)
        assert np.array_equal(_restored(got, "group_af"), grecs["af"], equal_nan=True)
        assert np.array_equal(got["group_total_depth"], grecs["total_depth"].astype(np.float64))


def test_dump_of_a_large_step_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 20)  # (the real limit: 64 MB)
    recs, _ = _records(20000, 0, 2)
    n = bench.dump_outputs(str(tmp_path / "a"), recs, None, 7)
    assert 0 < n < 20000 and bench.dump_outputs(str(tmp_path / "b"), recs, None, 7) == n
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    _same(a, b)  # same arguments, same sample
    assert sum(os.path.getsize(p) for p in glob.glob(str(tmp_path / "a" / "*.npy"))) <= 1 << 20
    idx = a["site_index"].astype(np.int64)
    assert len(idx) == n and (np.diff(idx) > 0).all() and idx[-1] < 20000
    assert np.array_equal(_restored(a, "qual"), recs["qual"][idx], equal_nan=True)


def _bench(out, extra=(), world=1):
    env = dict(os.environ)
    if world > 1:
        env.update(BASEVAR_BENCH_BACKEND="gloo", BASEVAR_BENCH_ONE_DEVICE="1")
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--dump-outputs", out] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), _load(out)


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_identically(tmp_path):
    """Two runs with the same arguments dump the same records: every site of the last step, float64, within 64 MB."""
    extra = ["--samples", "20000", "--batch-sites", "4096", "--groups", "2"]
    d, a = _bench(str(tmp_path / "a"), extra)
    _, b = _bench(str(tmp_path / "b"), extra)
    _same(a, b)
    assert d["steps"] == 2 and d["roofline"]["launches"] == 2
    assert np.array_equal(a["site_index"], np.arange(4096)) and a["group_af"].shape == (4096, 2, 4)
    assert all(v.dtype in (np.float64, np.float32) and np.isfinite(v).all() for v in a.values())
    assert (a["bq_ranksum_nonfinite"] == 1).any()  # sites without a variant: no rank sums (NaN in the records)
    assert sum(os.path.getsize(p) for p in glob.glob(str(tmp_path / "a" / "*.npy"))) <= 64 * 10 ** 6
    assert (a["total_depth"] > 0).all() and int(((a["status"].astype(np.int64) & 2) != 0).sum()) == d["config"]["variant_sites_last_batch"]


@pytest.mark.gpu
def test_bench_dump_outputs_gathered_over_two_ranks(tmp_path):
    """At N > 1 rank 0 dumps the gathered records of every rank: rank 0's part equals the one-rank run's records."""
    extra = ["--samples", "20000", "--batch-sites", "2048", "--distinct-batches", "1"]
    _, one = _bench(str(tmp_path / "one"), extra)
    d, two = _bench(str(tmp_path / "two"), extra, world=2)
    assert d["config"]["gathered_records_ok"] is True and len(two["site_index"]) == 2 * 2048
    for k in one:
        if k != "site_index":
            assert np.array_equal(two[k][:2048], one[k], equal_nan=True), k
