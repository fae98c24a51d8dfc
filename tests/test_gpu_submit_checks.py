"""The row-submit entry points of the C ABI (csrc/bv_engine_rows.hip): what they refuse and why, and the scratch that grows
with what they accept.

1. bv_engine_submit and bv_engine_submit_many(_g) refuse the same slabs with the same code for the same reason (one check,
   check_slab), before anything is queued: a valid submit on the same engine afterwards writes the records of a fresh engine.
2. One engine, given small, large and small slabs again on every scratch-growing path, writes what a fresh engine per slab writes.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from basevar_amd.synth import make_slab


@pytest.fixture(scope="module")
def bv():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import basevar_amd
    return basevar_amd


class DevSlab:
    """A make_slab() slab in device memory, with record buffers of its own."""

    def __init__(self, bv, slab, gid_t=None, n_groups=0, rows=None):
        import torch
        dev = torch.device("cuda", 0)
        rows = slice(None) if rows is None else rows
        self.n_sites = int(slab["base_strand"][rows].shape[0])
        self.pitch = int(slab["pitch"])
        self.n_samples = int(slab.get("n_samples", self.pitch))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.bs, self.q, self.mapq, self.ref = (up(slab[k][rows]) for k in ("base_strand", "qual", "mapq", "ref_base"))
        self.rpr = up(np.ascontiguousarray(slab["rpr"][rows]).view(np.int16))
        self.gid, self.n_groups = gid_t, n_groups
        self.out = torch.zeros(self.n_sites * bv.SITE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.gout = torch.zeros(max(1, self.n_sites * n_groups * bv.GROUP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def seg(self):
        return (self.n_sites, self.bs.data_ptr(), self.q.data_ptr(), self.ref.data_ptr(), self.out.data_ptr(), self.mapq.data_ptr(),
                self.rpr.data_ptr())

    def clear(self):
        self.out.zero_()
        self.gout.fill_(0xEE)

    def submit(self, eng):
        self.clear()
        eng.submit_ptrs(self.n_sites, self.n_samples, self.pitch, self.bs.data_ptr(), self.q.data_ptr(), self.ref.data_ptr(),
                        self.out.data_ptr(), self.mapq.data_ptr(), self.rpr.data_ptr(), group_id=self.gid.data_ptr() if self.n_groups else 0,
                        n_groups=self.n_groups, gout=self.gout.data_ptr() if self.n_groups else 0)
        eng.wait()
        return self.records()

    def records(self):
        """(site records, group records) as bytes"""
        return self.out.cpu().numpy().tobytes(), (self.gout.cpu().numpy().tobytes() if self.n_groups else b"")

    def fresh(self, bv, maf):
        """what a fresh engine of this slab's size writes (computed once)"""
        if not hasattr(self, "_fresh"):
            eng = bv.BaseTypeEngine(max_sites=self.n_sites, min_af_value=maf, device=0)
            self._fresh = self.submit(eng)
            eng.close()
        return self._fresh


# ---- 1. the refusals ------------------------------------------------------------------------------------------------------------
N1, S1, MAX1 = 64, 4, 8
INVALID, TOO_LARGE = -1, -4   # BV_ERR_INVALID_ARG, BV_ERR_TOO_LARGE (include/basevar_amd.h)
PITCH = "pitch must be >= n_samples and a multiple of 16"
PLANES = "base_strand, qual and ref_base planes are required"
TOGETHER = "mapq and rpr planes must be given together"
NEEDS = "n_groups > 0 needs group_id and gout"
# (id, what to change in the good slab -- bv_slab fields; "+field": bytes added to that pointer; out / gout: the record buffers --,
#  code, reason).  "GID" / "GOUT": a valid device group_id array / group record buffer.
DEFECTS = [
    ("n_sites_0", {"n_sites": 0}, INVALID, "n_sites == 0"),
    ("n_sites_above_max_sites", {"n_sites": MAX1 + 1}, TOO_LARGE, "n_sites exceeds cfg.max_sites"),
    ("pitch_below_n_samples", {"pitch": 48}, INVALID, PITCH),
    ("pitch_not_multiple_of_16", {"pitch": 72}, INVALID, PITCH),
    ("no_base_strand", {"base_strand": None}, INVALID, PLANES),
    ("no_qual", {"qual": None}, INVALID, PLANES),
    ("no_ref_base", {"ref_base": None}, INVALID, PLANES),
    ("mapq_without_rpr", {"rpr": None}, INVALID, TOGETHER),
    ("rpr_without_mapq", {"mapq": None}, INVALID, TOGETHER),
    ("n_groups_above_max", {"n_groups": 256, "group_id": "GID", "gout": "GOUT"}, INVALID, "n_groups exceeds BV_MAX_GROUPS"),
    ("groups_without_group_id", {"n_groups": 2, "gout": "GOUT"}, INVALID, NEEDS),
    ("groups_without_gout", {"n_groups": 2, "group_id": "GID", "gout": None}, INVALID, NEEDS),
    ("plane_misaligned", {"+qual": 8}, INVALID, "planes must be 16-byte aligned"),
    ("rank_plane_misaligned", {"+rpr": 2}, INVALID, "planes must be 16-byte aligned"),
    ("records_misaligned", {"+out": 8}, INVALID, "device record buffers must be 16-byte aligned"),
    ("unknown_layout_bit", {"layout": 0x2}, INVALID, "unknown bv_slab.layout bits"),
    ("reserved_nonzero", {"reserved_": 1}, INVALID, "unknown bv_slab.layout bits"),
]


@pytest.fixture(scope="module")
def good(bv):
    import torch
    slab = make_slab(S1, N1, seed=41, coverage=0.5, class_af=[(0.3, 0.0), (0.0, 0.0), (0.2, 0.2)])
    assert slab["pitch"] == 64
    d = DevSlab(bv, slab)
    d.maf = bv.min_af(N1)
    d.gid_valid = torch.zeros(N1, dtype=torch.uint8, device=torch.device("cuda", 0))
    d.gout_valid = torch.zeros(S1 * 2 * bv.GROUP_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", 0))
    base = d.fresh(bv, d.maf)
    assert (np.frombuffer(base[0], bv.SITE_DTYPE)["status"] & 2).any()
    return d


@pytest.mark.parametrize("change,code,reason", [d[1:] for d in DEFECTS], ids=[d[0] for d in DEFECTS])
def test_both_entry_points_refuse_a_slab_for_the_same_reason(bv, good, change, code, reason):
    from basevar_amd import _capi
    lib = _capi.load()
    eng = bv.BaseTypeEngine(max_sites=MAX1, min_af_value=good.maf, device=0)
    ok = _capi.Slab(S1, N1, 64, good.bs.data_ptr(), good.q.data_ptr(), good.mapq.data_ptr(), good.rpr.data_ptr(), good.ref.data_ptr(),
                    None, 0, _capi.BV_MEM_DEVICE, 0)
    bad = _capi.Slab.from_buffer_copy(ok)
    out, gout, with_gout = good.out.data_ptr(), None, False
    for k, v in change.items():
        v = {"GID": good.gid_valid.data_ptr(), "GOUT": good.gout_valid.data_ptr()}.get(v, v) if isinstance(v, str) else v
        if k == "gout":
            gout, with_gout = v, True
        elif k == "+out":
            out += v
        elif k[0] == "+":
            setattr(bad, k[1:], getattr(bad, k[1:]) + v)
        else:
            setattr(bad, k, v)
    good.clear()
    # bv_engine_submit
    rc = lib.bv_engine_submit(eng._h, C.byref(bad), out, gout, None)
    msg = eng._err()
    assert rc == code, msg
    assert msg.startswith("bv_engine_submit: " + reason), msg
    # bv_engine_submit_many(_g): the good slab first, the bad one second
    arr = (_capi.Slab * 2)(ok, bad)
    outs = (C.c_void_p * 2)(good.out.data_ptr(), out)
    if with_gout:
        rc = lib.bv_engine_submit_many_g(eng._h, 2, arr, outs, (C.c_void_p * 2)(None, gout), None)
    else:
        rc = lib.bv_engine_submit_many(eng._h, 2, arr, outs, None)
    msg = eng._err()
    assert rc == code, msg
    assert msg.startswith("bv_engine_submit_many: slab 1: " + reason), msg
    # nothing was queued, no state was left behind: the good slab's records are untouched, and a valid submit writes a fresh engine's
    eng.wait()
    assert good.records()[0] == bytes(len(good.fresh(bv, good.maf)[0]))
    assert good.submit(eng) == good.fresh(bv, good.maf)
    eng.close()


# ---- 2. the scratch ---------------------------------------------------------------------------------------------------------------
MAX2 = 320


@pytest.fixture(scope="module")
def engine2(bv):
    """ONE engine for the four steps below, in the order of the file: its scratch has seen what the steps before have left"""
    eng = bv.BaseTypeEngine(max_sites=MAX2, min_af_value=bv.min_af(4100), device=0)
    yield eng
    eng.close()


def slabs_of(bv, n, groups=0, sizes=(16, 300, 16)):
    import torch
    gid_t = None
    if groups:
        g = np.random.default_rng(n + groups).integers(0, groups + 1, size=(n + 15) // 16 * 16).astype(np.uint8)
        g[g == groups] = 255  # in no group
        gid_t = torch.from_numpy(g).to(torch.device("cuda", 0))
    return [DevSlab(bv, make_slab(s, n, seed=7000 + n + 10 * k + groups, coverage=0.08, class_af=[(0.0, 0.0), (0.3, 0.0), (0.2, 0.1)]),
                    gid_t, groups) for k, s in enumerate(sizes)]


@pytest.mark.parametrize("n,groups,form", [(4100, 0, 0x7), (300, 0, 0x1), (4100, 3, 0x7)], ids=["fused_kernel", "streaming_and_solve_kernels", "pop_groups"])
def test_scratch_regrows_and_is_reused(bv, engine2, n, groups, form):
    """16, then 300, then 16 sites on one engine of max_sites 320: the short-row scratch (and with pop-groups the item scratch and
    the prepared group plane) grows for the second slab and is reused, larger than needed, by the third.  The min_af of the
    engine is that of 4,100 samples throughout (the fresh engines': the same)."""
    maf = engine2.min_af
    n_var = 0
    for k, d in enumerate(slabs_of(bv, n, groups)):
        want = d.fresh(bv, maf)
        got = d.submit(engine2)
        assert engine2.last_launch_form() == form  # BV_FORM_SHORT_ROWS | ONE_KERNEL | PASS2_FUSED (include/basevar_amd_diag.h)
        assert got[0] == want[0], "slab %d" % k
        assert got[1] == want[1], "pop-group records of slab %d" % k
        n_var += int((np.frombuffer(got[0], bv.SITE_DTYPE)["status"] & 2 != 0).sum())
    assert n_var > 50


def test_chained_slabs_after_the_single_ones(bv, engine2):
    """One chained submit_many of three 4,100-sample slabs (16 + 280 + 16 sites: together within max_sites) on the engine the
    single submits have used: the contiguous copies of the reference bases and the records are made on first use."""
    maf = engine2.min_af
    a, b, c = slabs_of(bv, 4100)
    big = make_slab(300, 4100, seed=7000 + 4100 + 10, coverage=0.08, class_af=[(0.0, 0.0), (0.3, 0.0), (0.2, 0.1)])
    b = DevSlab(bv, big, rows=slice(0, 280))
    ds = [a, b, c]
    want = [d.fresh(bv, maf) for d in ds]
    for d in ds:
        d.clear()
    engine2.submit_many_ptrs(4100, a.pitch, [d.seg() for d in ds])
    engine2.wait()
    for k, d in enumerate(ds):
        assert d.records()[0] == want[k][0], "slab %d" % k
    assert engine2.last_variant_count() == sum(int((np.frombuffer(w[0], bv.SITE_DTYPE)["status"] & 2 != 0).sum()) for w in want) > 50
