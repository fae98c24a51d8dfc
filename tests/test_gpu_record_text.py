"""GPU tests of bv_engine_cvg_format and bv_engine_vcf_format_records (include/basevar_amd_record_text.h): the CVG rows and the
VCF heads the device writes from the records are, byte for byte, those of host/vcf_emit.hpp's format_cvg_line and format_vcf_head
-- printed by the stand-alone harness tests/cpp/record_text_check.cpp -- and of the serial model tests/record_text_model.py, at
every line count, alignment, CHROM length and group count at which the kernels of basevar_amd/csrc/bv_record_text.hip take
another path; whole VCF lines are bv_engine_vcf_format's for the same heads; records outside the domain are refused or go as
host text."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import record_text_model as model  # noqa: E402
import record_text_ref as ref  # noqa: E402

SENTINEL = 0xA5
NOCALL_TAIL = b"\t./.\n"  # a VCF line's one sample column over a row whose only cell is uncovered


@pytest.fixture(scope="module")
def harness():
    return ref.build()


@pytest.fixture(scope="module")
def eng():
    import basevar_amd as bv
    e = bv.BaseTypeEngine(max_sites=64, min_af_value=bv.min_af(2048), device=0, max_samples=2048)
    yield e
    e.close()


def names_of(n_groups):
    return [(b"G%d" % j) * (1 + j % 3) for j in range(n_groups)]


def arrays(lines, n_groups):
    from basevar_amd import _capi
    sites = np.array([ln["rec"] for ln in lines], dtype=_capi.SITE_DTYPE)
    groups = np.array([ln["groups"] for ln in lines], dtype=_capi.GROUP_DTYPE).reshape(len(lines), n_groups) if n_groups else None
    return sites, groups, np.array([ln["pos"] for ln in lines], np.uint32), b"".join(ln["ref"][:1] for ln in lines)


def on_device_memory(sites, groups):
    """the records in device memory: ((pointer, n), (pointer, n_groups) or None) and what keeps them alive"""
    import torch
    ts = torch.from_numpy(np.frombuffer(sites.tobytes(), np.uint8).copy()).cuda()
    tg = torch.from_numpy(np.frombuffer(groups.tobytes(), np.uint8).copy()).cuda() if groups is not None and groups.size else None
    torch.cuda.synchronize()
    return (int(ts.data_ptr()), len(sites)), ((int(tg.data_ptr()), groups.shape[1]) if tg is not None else None), (ts, tg)


def one_cell_slab(n_rows=1):
    """rows of one uncovered sample each, on the device"""
    import torch
    from basevar_amd import _capi
    cell = torch.full((n_rows, 16), 8, dtype=torch.uint8).cuda()
    phred = torch.zeros((n_rows, 16), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return _capi.Slab(n_rows, 1, 16, int(cell.data_ptr()), int(phred.data_ptr()), None, None, None, None, 0, _capi.BV_MEM_DEVICE, 0, 0), (cell, phred)


def offsets(texts):
    off = np.zeros(len(texts) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in texts])
    return off


def check_both(eng, harness, tmp_path, lines, n_groups, device_records=False, host_lines=()):
    """cvg_format and vcf_format_records (over one uncovered sample) of `lines` against the harness's dump and the model.
    Lines the predicate refuses, and those of `host_lines`, go as host text.  Returns the expected CVG and VCF texts."""
    names = names_of(n_groups)
    dump = ref.run_lines(harness, lines, names, tmp_path)
    chrom = lines[0]["chrom"]
    assert all(ln["chrom"] == chrom for ln in lines)
    sites, groups, pos, refs = arrays(lines, n_groups)
    for ln, (on, gt, vcf, cvg, indel) in zip(lines, dump):
        if on:
            g = ln["groups"] if n_groups else ()
            assert model.vcf_head(ln["rec"], g, names, chrom, ln["pos"], ln["ref"]) == vcf
            assert model.cvg_row(ln["rec"], chrom, ln["pos"], ln["ref"], b"" if indel == b"." else indel) == cvg
    as_host = [(not on) or k in host_lines for k, (on, *_) in enumerate(dump)]
    cvg_host = [d[3] if h else None for d, h in zip(dump, as_host)]
    vcf_host = [d[2] if h else None for d, h in zip(dump, as_host)]
    indel = [None if d[4] == b"." else d[4] for d in dump]
    keep = None
    rec_arg, grp_arg = sites, groups
    if device_records:
        rec_arg, grp_arg, keep = on_device_memory(sites, groups)
    cvg_rows = [d[3] for d in dump]
    off = eng.cvg_format(rec_arg, chrom, pos, refs, indel=indel, host_text=cvg_host, groups=grp_arg, group_names=names)
    assert np.array_equal(off, offsets(cvg_rows))
    assert eng.cvg_fetch().tobytes() == b"".join(cvg_rows)
    slab, keep_slab = one_cell_slab()
    vcf_lines = [d[2] + NOCALL_TAIL if d[2] else b"" for d in dump]
    off = eng.vcf_format_records(np.zeros(len(lines), np.uint32), rec_arg, chrom, pos, refs, groups=grp_arg, group_names=names, host_text=vcf_host, slab=slab)
    assert np.array_equal(off, offsets(vcf_lines))
    assert eng.vcf_fetch().tobytes() == b"".join(vcf_lines)
    del keep, keep_slab
    return cvg_rows, vcf_lines


@pytest.mark.parametrize("device_records", [False, True])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_line_counts(eng, harness, tmp_path, n, device_records):
    lines = ref.seeded_lines(500 + n, n, 2, chrom=b"chr22")
    for ln in lines[:3]:  # (the first lines have text, whatever the seed)
        ln["rec"]["total_depth"] = max(int(ln["rec"]["total_depth"]), 1)
    check_both(eng, harness, tmp_path, lines, 2, device_records)


def test_chrom_lengths_and_every_alignment(eng, harness, tmp_path):
    """CHROM of 1 .. 40 bytes; over the calls, rows and heads begin at every offset modulo 16 (asserted from the expected text)"""
    cvg_res, vcf_res = set(), set()
    for n_chrom in range(1, 41):
        lines = ref.seeded_lines(900 + n_chrom, 24, 1, chrom=bytes(np.random.default_rng(n_chrom).integers(65, 91, n_chrom).astype(np.uint8)))
        cvg, vcf = check_both(eng, harness, tmp_path, lines, 1)
        cvg_res |= {int(o) % 16 for o, t in zip(offsets(cvg), cvg) if t}
        vcf_res |= {int(o) % 16 for o, t in zip(offsets(vcf), vcf) if t}
    assert cvg_res == set(range(16)) and vcf_res == set(range(16))


@pytest.mark.parametrize("n_groups", [0, 1, 2, 21, 22, 40, 255])
def test_group_counts(eng, harness, tmp_path, n_groups):
    """13 groups give the 64th item, 21 the first step of a second 64; 255 groups are 791 items"""
    lines = ref.seeded_lines(700 + n_groups, 20, n_groups, chrom=b"chrX")
    for ln in lines[:4]:
        if int(ln["rec"]["n_alt"]) and n_groups:
            ln["groups"]["n_alt"] = int(ln["rec"]["n_alt"])  # every group prints, with every AF
            ln["groups"]["af"][:, :int(ln["rec"]["n_alt"])] = 0.125
    check_both(eng, harness, tmp_path, lines, n_groups, device_records=n_groups in (22, 255))


def test_empty_lines_first_last_and_between(eng, harness, tmp_path):
    rng = np.random.default_rng(5)
    lines = []
    for k, kind in enumerate("eexeexxeexe"):
        r, g = ref.record(rng, [1, 3] if kind == "x" else [], 1)
        if kind == "e":
            r["total_depth"] = 0
        lines.append(ref.line(r, g, chrom=b"c", pos=k + 1, ref=b"g"))
    cvg, vcf = check_both(eng, harness, tmp_path, lines, 1)
    assert [bool(t) for t in cvg] == [k == "x" for k in "eexeexxeexe"] == [bool(t) for t in vcf]
    only_empty = [ln for ln in lines if int(ln["rec"]["total_depth"]) == 0]
    cvg, vcf = check_both(eng, harness, tmp_path, only_empty, 1)
    assert b"".join(cvg) == b"" == b"".join(vcf)


@pytest.mark.parametrize("device_records", [False, True])
def test_host_text_lines_among_device_lines(eng, harness, tmp_path, device_records):
    """lines 0, 1, 62, 63 and 64 come as host text, three of them because their record has a NaN AF"""
    lines = ref.seeded_lines(41, 130, 2, chrom=b"chr7")
    for k in (0, 1, 62, 63, 64):
        r, g = ref.record(np.random.default_rng(k), [0, 2], 2)
        if k in (0, 63, 64):
            r["af"][0] = np.nan
        lines[k] = ref.line(r, g, chrom=b"chr7", pos=k + 5, ref=b"T", tokens=[b"+A"] if k == 1 else ())
    check_both(eng, harness, tmp_path, lines, 2, device_records, host_lines=(0, 1, 62, 63, 64))


def test_special_values_in_every_numeric_field(eng, harness, tmp_path):
    """the tie, carry and domain-edge values of the CPU corpus in every numeric field in turn; the values outside a domain make
    their records the host's"""
    lines = ref.special_lines(2)
    for ln in lines:
        ln["chrom"] = b"chrS"
    check_both(eng, harness, tmp_path, lines, 2)


def test_fetch_leaves_its_surroundings(eng, harness, tmp_path):
    import torch
    lines = ref.seeded_lines(77, 65, 2, chrom=b"chr1")
    dump = ref.run_lines(harness, lines, names_of(2), tmp_path)
    sites, groups, pos, refs = arrays(lines, 2)
    off = eng.cvg_format(sites, b"chr1", pos, refs, indel=[None if d[4] == b"." else d[4] for d in dump], groups=groups, group_names=names_of(2))
    want = b"".join(d[3] for d in dump)
    size = int(off[-1])
    assert size == len(want)
    buf = torch.full((size + 64,), SENTINEL, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert eng.cvg_fetch(dst_ptr=int(buf.data_ptr()) + 32, dst_capacity=size) is None
    got = buf.cpu().numpy()
    assert (got[:32] == SENTINEL).all() and (got[32 + size:] == SENTINEL).all() and got[32:32 + size].tobytes() == want
    for level in ("fast", "small"):
        members, moff = eng.cvg_deflate(level=level)
        ref_members, ref_moff = eng.bgzf_deflate(want, level=level)
        assert np.array_equal(moff, ref_moff) and members.tobytes() == ref_members.tobytes()


def sample_planes(rng, n_rows, n):
    cell = np.where(rng.random((n_rows, n)) < 0.3, rng.integers(0, 8, (n_rows, n)), rng.choice([8, 9, 10], (n_rows, n))).astype(np.uint8)
    return cell, rng.integers(0, 256, (n_rows, n)).astype(np.uint8)


@pytest.mark.parametrize("device_slab", [False, True])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025])
def test_whole_lines_are_vcf_formats(eng, harness, tmp_path, n, device_slab):
    """vcf_format_records == vcf_format given the model's heads and gt characters, the same text byte for byte, and its
    members are bgzf_deflate's of that text at both levels"""
    from test_gpu_vcf_lines import Padded
    rng = np.random.default_rng(n)
    n_rows = 12
    cell, phred = sample_planes(rng, n_rows, n)
    lines = [ln for ln in ref.seeded_lines(3000 + n, 40, 2, chrom=b"chr9")]
    names = names_of(2)
    site = rng.integers(0, n_rows, len(lines)).astype(np.uint32)
    sites, groups, pos, refs = arrays(lines, 2)
    P = Padded(cell, phred)
    slab = P.slab(device_slab)
    off = eng.vcf_format_records(site, sites, b"chr9", pos, refs, groups=groups, group_names=names, slab=slab)
    got = eng.vcf_fetch().tobytes()
    deflated = {level: eng.vcf_deflate(level=level) for level in ("fast", "small")}
    has = [k for k, ln in enumerate(lines) if int(ln["rec"]["n_alt"])]
    assert 0 < len(has) < len(lines)
    heads = [model.vcf_head(lines[k]["rec"], lines[k]["groups"], names, b"chr9", lines[k]["pos"], lines[k]["ref"]) for k in has]
    gt = np.array([list(model.gt_codes(lines[k]["rec"], lines[k]["ref"])) for k in has], np.uint8)
    want_off = eng.vcf_format(site[has], heads, gt, slab)
    want = eng.vcf_fetch().tobytes()
    assert got == want
    assert np.array_equal(off[np.array(has + [len(lines)])], want_off) and int(off[0]) == 0
    assert all(int(off[k + 1]) == int(off[k]) for k in range(len(lines)) if k not in has)
    for level, (members, moff) in deflated.items():
        ref_members, ref_moff = eng.bgzf_deflate(want, level=level)
        assert np.array_equal(moff, ref_moff) and members.tobytes() == ref_members.tobytes()


def test_rows_kept_by_lrt_text(harness, tmp_path):
    """slab == NULL: the lines of every record of a parsed batch, from the rows and over the records lrt_text left"""
    import basevar_amd as bv
    from basevar_amd.synth import make_slab
    from test_gpu_text_rows import _py_host_reader, slab_rows
    fs = [200, 120, 37]
    P, N, F = 30, sum(fs), 3
    slab = make_slab(P, N, seed=309, coverage=0.1, indel_frac=0.02, n_groups=2)
    text, off = slab_rows(slab, fs, depth_zero=(2, 11))
    rows = [[bytes(text[int(off[p * F + f]):int(off[p * F + f + 1]) - 1]) for f in range(F)] for p in range(P)]
    e = bv.BaseTypeEngine(max_sites=P, min_af_value=bv.min_af(N), device=0, max_samples=N)
    try:
        tb = e.lrt_text(rows, fs, group_id=slab["group_id"], n_groups=2, host_reader=_py_host_reader(N))
        n = len(tb.sites)
        names = [b"G0", b"G1"]
        pos = np.array([int(rows[int(p)][0].split(b"\t")[1]) for p in tb.positions], np.uint32)
        refs = b"".join(rows[int(p)][0].split(b"\t")[2][:1] for p in tb.positions)
        chrom = rows[0][0].split(b"\t")[0]
        ok = bv.BaseTypeEngine.record_text_on_device(tb.sites, tb.groups)
        host = [None if ok[k] else b"HOST\tHEAD\t%d" % k for k in range(n)]
        line_off = e.vcf_format_records(np.arange(n, dtype=np.uint32), tb.sites, chrom, pos, refs, groups=tb.groups, group_names=names, host_text=host)
        got = e.vcf_fetch().tobytes()
        has = [k for k in range(n) if int(tb.sites[k]["n_alt"]) or not ok[k]]
        assert len(has) >= 3 and ok.sum() >= 3
        heads = [host[k] or model.vcf_head(tb.sites[k], tb.groups[k], names, chrom, pos[k], refs[k:k + 1]) for k in has]
        gt = np.array([list(model.gt_codes(tb.sites[k], refs[k:k + 1])) for k in has], np.uint8)
        want_off = e.vcf_format(np.array(has, np.uint32), heads, gt, None)
        assert got == e.vcf_fetch().tobytes() and int(line_off[-1]) == int(want_off[-1])
    finally:
        e.close()


def test_refusals(eng, harness, tmp_path):
    from basevar_amd import _capi
    lines = ref.seeded_lines(9, 8, 1, chrom=b"chr1")
    for ln in lines:
        ln["rec"]["total_depth"] = max(1, int(ln["rec"]["total_depth"]))
    names = names_of(1)
    sites, groups, pos, refs = arrays(lines, 1)
    slab, keep = one_cell_slab()
    site = np.zeros(len(lines), np.uint32)

    def both(match, code, **change):
        kw = dict(sites=sites, groups=groups, pos=pos, refs=refs, chrom=b"chr1", names=names, host_text=None)
        kw.update(change)
        for call in ("cvg", "vcf"):
            with pytest.raises(RuntimeError, match=match) as ei:
                if call == "cvg":
                    eng.cvg_format(kw["sites"], kw["chrom"], kw["pos"], kw["refs"], groups=kw["groups"], group_names=kw["names"], host_text=kw["host_text"])
                else:
                    eng.vcf_format_records(site, kw["sites"], kw["chrom"], kw["pos"], kw["refs"], groups=kw["groups"], group_names=kw["names"],
                                           host_text=kw["host_text"], slab=slab)
            assert ei.value.args[1] == code, ei.value.args

    # a good call first: its texts must not survive a refused record
    eng.cvg_format(sites, b"chr1", pos, refs, groups=groups, group_names=names)
    eng.vcf_format_records(site, sites, b"chr1", pos, refs, groups=groups, group_names=names, slab=slab)
    assert eng.cvg_fetch().size and eng.vcf_fetch().size
    # outside the domain, without host text: BV_ERR_DATA, the line and the field named, no text held
    bad = sites.copy()
    bad[5]["n_alt"], bad[5]["alt"][0] = max(1, int(bad[5]["n_alt"])), 2
    bad[5]["qual"] = np.inf
    bad[5]["cvg_sor"] = np.nan
    with pytest.raises(RuntimeError, match="line 5, field SOR") as ei:
        eng.cvg_format(bad, b"chr1", pos, refs, groups=groups, group_names=names)
    assert ei.value.args[1] == _capi.BV_ERR_DATA
    with pytest.raises(RuntimeError, match="line 5, field QUAL") as ei:
        eng.vcf_format_records(site, bad, b"chr1", pos, refs, groups=groups, group_names=names, slab=slab)
    assert ei.value.args[1] == _capi.BV_ERR_DATA
    for fetch in ("bv_engine_cvg_fetch", "bv_engine_vcf_fetch"):
        buf = np.zeros(1 << 16, np.uint8)
        assert getattr(eng._lib, fetch)(eng._h, buf.ctypes.data, buf.size, _capi.BV_MEM_HOST, None) == _capi.BV_ERR_INVALID_ARG
    dev_rec, dev_grp, keep_dev = on_device_memory(bad, groups)
    with pytest.raises(RuntimeError, match="line 5, field SOR"):
        eng.cvg_format(dev_rec, b"chr1", pos, refs, groups=dev_grp, group_names=names)
    # what the host checks before a launch: BV_ERR_INVALID_ARG
    many = sites.copy()
    many[2]["n_alt"] = 4
    both("line 2: n_alt 4 > 3", _capi.BV_ERR_INVALID_ARG, sites=many)
    code = sites.copy()
    code[3]["n_alt"], code[3]["alt"][0] = 1, 4
    both("line 3: alt code 4 above 3", _capi.BV_ERR_INVALID_ARG, sites=code)
    gcode = groups.copy()
    gcode[1, 0]["n_alt"], gcode[1, 0]["alt"][0] = 1, 7
    both("line 1, group 0: alt code 7", _capi.BV_ERR_INVALID_ARG, groups=gcode)
    dev_rec, dev_grp, keep_dev2 = on_device_memory(code, groups)
    both("line 3: a record with more ALTs", _capi.BV_ERR_INVALID_ARG, sites=dev_rec, groups=dev_grp)
    both("chrom_len", _capi.BV_ERR_INVALID_ARG, chrom=b"")
    both("chrom_len", _capi.BV_ERR_INVALID_ARG, chrom=b"c" * 256)
    both("name of group 0", _capi.BV_ERR_INVALID_ARG, names=[b"n" * 256])
    lib, h = eng._lib, eng._h
    line_off = np.zeros(len(lines) + 1, np.uint64)

    def raw(**change):
        L, keep_l, _ = eng._record_lines("test", sites, groups, b"chr1", pos, refs, names, None, len(lines))
        L.site, L.slab = site.ctypes.data, C.pointer(slab)
        for k, v in change.items():
            setattr(L, k, v)
        out = []
        for fn in (lib.bv_engine_cvg_format, lib.bv_engine_vcf_format_records):
            line_off[:] = 7
            out.append(fn(h, C.byref(L), line_off.ctypes.data, None))
            assert out[-1] == _capi.BV_OK or (line_off == 7).all()  # a refusal leaves it unwritten
        return out
    assert raw(reserved_=1) == [_capi.BV_ERR_INVALID_ARG] * 2
    assert raw(mem_kind=2) == [_capi.BV_ERR_INVALID_ARG] * 2
    assert raw(records=None) == [_capi.BV_ERR_INVALID_ARG] * 2
    assert raw(pos=None) == [_capi.BV_ERR_INVALID_ARG] * 2
    assert raw(ref_char=None) == [_capi.BV_ERR_INVALID_ARG] * 2
    assert raw(chrom=None) == [_capi.BV_ERR_INVALID_ARG] * 2
    assert raw(groups=None) == [_capi.BV_ERR_INVALID_ARG] * 2
    assert raw(group_name_off=None) == [_capi.BV_ERR_INVALID_ARG] * 2
    assert raw(site=None)[1] == _capi.BV_ERR_INVALID_ARG
    disorder = np.array([0, 5, 3] + [3] * (len(lines) - 2), np.uint64)
    text = np.zeros(16, np.uint8)
    assert raw(host_text_off=disorder.ctypes.data, host_text=text.ctypes.data) == [_capi.BV_ERR_INVALID_ARG] * 2
    assert raw(indel_off=disorder.ctypes.data, indel=text.ctypes.data)[0] == _capi.BV_ERR_INVALID_ARG
    long_indel = np.array([0] + [_capi.RECORD_TEXT_INDEL_MAX + 1] * len(lines), np.uint64)
    big = np.zeros(_capi.RECORD_TEXT_INDEL_MAX + 1, np.uint8)
    assert raw(indel_off=long_indel.ctypes.data, indel=big.ctypes.data)[0] == _capi.BV_ERR_INVALID_ARG
    assert lib.bv_engine_cvg_format(h, None, line_off.ctypes.data, None) == _capi.BV_ERR_INVALID_ARG
    L, keep_l, _ = eng._record_lines("test", sites, groups, b"chr1", pos, refs, names, None, len(lines))
    assert lib.bv_engine_cvg_format(h, C.byref(L), None, None) == _capi.BV_ERR_INVALID_ARG
    assert lib.bv_engine_vcf_format_records(h, C.byref(L), line_off.ctypes.data, None) == _capi.BV_ERR_INVALID_ARG  # no site, no slab
    # no lines: BV_OK and an empty text
    assert np.array_equal(eng.cvg_format(sites[:0], b"chr1", pos[:0], b""), [0]) and eng.cvg_fetch().size == 0
    assert np.array_equal(eng.vcf_format_records(site[:0], sites[:0], b"chr1", pos[:0], b"", slab=slab), [0]) and eng.vcf_fetch().size == 0
    # and the engine still formats
    check_both(eng, harness, tmp_path, lines, 1)
    del keep, keep_dev, keep_dev2


def test_through_lrt_pileup_on_the_bam_corpus(harness, tmp_path):
    """the records and the gathered rows of a piled-up window of tests/test_gpu_pileup.py's corpus, where they lie: the CVG rows
    are the host formatter's, the VCF lines are vcf_format's given the host formatter's heads"""
    import pileup_ref as pr
    from test_gpu_pileup import engine as pileup_engine
    cdir = tmp_path / "corpus"
    cdir.mkdir()
    corpus = pr.Corpus(cdir, 65)
    w = pr.WINDOWS["w1000"]
    d = pr.run_bam(pr.build(), tmp_path / "w1000.bin", corpus, 65, w)[0]
    e = pileup_engine(corpus, n=65)
    try:
        got = e.lrt_pileup(d.records, d.run_off, d.run_sample, d.n_samples, d.tid, pr.REGION, w, pr.MAPQ_THD, tagged=True)
        slab, pos, depth = e.pileup_rows(tagged=True)
        n = len(got.sites)
        assert n == d.n_covered > 500
        by_pos = {}
        for (p, s), text in sorted(got.tokens.items()):
            by_pos.setdefault(p, []).append(text)
        lines = [ref.line(got.sites[k], None, chrom=b"chr1", pos=int(pos[k]), ref=corpus.fa[int(pos[k]) - 1].encode(), tokens=by_pos.get(int(pos[k]), ()))
                 for k in range(n)]
        dump = ref.run_lines(harness, lines, (), tmp_path)
        assert sum(1 for x in dump if x[4] != b".") >= 3 and sum(1 for x in dump if x[2]) >= 10
        refs = b"".join(ln["ref"] for ln in lines)
        off = e.cvg_format(got.sites, b"chr1", pos, refs, indel=[None if x[4] == b"." else x[4] for x in dump], host_text=[None if x[0] else x[3] for x in dump])
        assert e.cvg_fetch().tobytes() == b"".join(x[3] for x in dump) and int(off[-1]) == sum(len(x[3]) for x in dump)
        line_off = e.vcf_format_records(np.arange(n, dtype=np.uint32), got.sites, b"chr1", pos, refs, host_text=[None if x[0] else x[2] for x in dump], slab=slab)
        text = e.vcf_fetch().tobytes()
        has = [k for k in range(n) if dump[k][2]]
        want_off = e.vcf_format(np.array(has, np.uint32), [dump[k][2] for k in has], np.array([list(dump[k][1]) for k in has], np.uint8), slab)
        assert text == e.vcf_fetch().tobytes() and np.array_equal(line_off[np.array(has + [n])], want_off)
    finally:
        e.close()
