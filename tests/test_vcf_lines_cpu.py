"""CPU tests (no GPU) of the VCF sample columns' definition: basevar_amd/csrc/bv_vcf_core.h's serial line builder -- the code
the kernels of bv_vcf.hip compile -- against host/vcf_emit.hpp's format_vcf_line, inside the stand-alone harness
tests/cpp/vcf_lines_check.cpp built with ASan + UBSan and run as a program; the new header against the ctypes layer; and the
kernels' resources."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vcf_lines_ref as vr  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from basevar_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def harness(lib):
    return vr.build(asan=True)


def check_lines(got, cell, phred, lines):
    """the harness has compared the core with format_vcf_line; here its output is held to the written definition and formula"""
    for (head, gt, text), ln in zip(got, lines):
        c, q = cell[ln["site"]], phred[ln["site"]]
        assert text == vr.py_line(head, gt, c, q)
        assert len(text) == len(head) + 4 * c.size + 13 * int(((c & 8) == 0).sum()) + 1
        assert text.startswith(head) and head.endswith(b"\tGT:AB:SO:BP")


def test_every_cell_value_and_phred(harness, tmp_path):
    """every cell value the planes hold (0-7, BV_CELL_N, _INS, _DEL) x every phred 0-255, under three REF / ALT settings"""
    rng = np.random.default_rng(11)
    cells = np.repeat(np.array(vr.CELL_VALUES, np.uint8), 256)[None, :]
    phred = np.tile(np.arange(256, dtype=np.uint8), len(vr.CELL_VALUES))[None, :]
    lines = [vr.line(0, vr.record(rng, alts)[0], ref_base=rb) for rb, alts in ((b"A", [1]), (b"g", [0, 3, 1]), (b"N", [3, 2]))]
    got = vr.run(harness, cells, phred, lines, tmp_dir=tmp_path)
    check_lines(got, cells, phred, lines)
    toks = got[0][2][len(got[0][0]):].rstrip(b"\n").split(b"\t")[1:]
    assert len(toks) == cells.size and set(toks[8 * 256:]) == {b"./."}
    bp = {t.rsplit(b":", 1)[-1] for t in toks[:256]}  # cell 0 at every phred
    assert all(len(x) == 8 for x in bp)  # every BP string is 8 characters
    assert b"0.000000" in bp and b"1.000000" in bp


def test_every_ref_base_and_alt_set(harness, tmp_path):
    """every REF base (upper and lower case, and two that are not ACGT) x every ordered ALT set of 1-3 bases"""
    rng = np.random.default_rng(12)
    cells = np.array([vr.CELL_VALUES * 3], np.uint8)
    phred = rng.integers(0, 256, cells.shape).astype(np.uint8)
    lines = []
    for rb in (b"A", b"C", b"G", b"T", b"a", b"t", b"N", b"R"):
        for k in (1, 2, 3):
            for alts in itertools.permutations(range(4), k):
                lines.append(vr.line(0, vr.record(rng, list(alts))[0], ref_base=rb, ref_pos=len(lines) + 1))
    got = vr.run(harness, cells, phred, lines, tmp_dir=tmp_path)
    check_lines(got, cells, phred, lines)
    seen = {bytes(gt) for _, gt, _ in got}
    assert {b"0123"[i:i + 1] for i in range(4)} | {b"."} == {bytes([c]) for s in seen for c in s}
    # an ALT that is the REF base keeps "0/." (caller.cpp:1136-1143): REF A, ALT A first -> A is '0', the next ALT is '2'
    a_first = [gt for (_, gt, _), ln in zip(got, lines) if ln["ref_base"] == b"A" and ln["rec"]["alt"][0] == 0 and ln["rec"]["n_alt"] == 2]
    assert a_first and all(gt[0] == ord("0") and sorted(gt.tolist()).count(ord("2")) == 1 for gt in a_first)


@pytest.mark.parametrize("n_groups", [0, 2])
def test_seeded_records(harness, tmp_path, n_groups):
    """seeded records as tests/cpp/emit_corpus.cpp draws them (coverage 0.08, one to three ALTs), with and without pop-groups"""
    rng = np.random.default_rng(13 + n_groups)
    n_rows, n = 24, 777
    cells = np.where(rng.random((n_rows, n)) < 0.08, rng.integers(0, 8, (n_rows, n)), rng.choice([8, 9, 10], (n_rows, n))).astype(np.uint8)
    phred = rng.integers(0, 64, (n_rows, n)).astype(np.uint8)
    names = [b"EAS", b"pop_2"][:n_groups]
    lines = []
    for k in range(40):
        ref = int(rng.integers(0, 4))
        alts = [(ref + 1 + int(a)) & 3 for a in rng.permutation(3)[:int(rng.integers(1, 4))]]
        rec, groups = vr.record(rng, alts, n_groups)
        lines.append(vr.line(int(rng.integers(0, n_rows)), rec, groups if n_groups else None, ref_base=vr.BASES[ref:ref + 1], ref_pos=10000 + 7 * k,
                             ref_id=b"chr%d" % (1 + k // 20)))
    got = vr.run(harness, cells, phred, lines, names, tmp_dir=tmp_path)
    check_lines(got, cells, phred, lines)
    if n_groups:
        assert any(b";EAS_AF=" in h for h, _, _ in got)
    # a head given in the record's place stands in front of the same columns
    with_head = [dict(ln, head=b"x" * (k + 1)) for k, ln in enumerate(lines[:5])]
    for (h, _, text), (h0, _, text0) in zip(vr.run(harness, cells, phred, with_head, names, tmp_dir=tmp_path), got):
        assert text[len(h):] == text0[len(h0):] and text.startswith(h) and len(h) < len(h0)


def test_harness_refuses_what_it_cannot_format(harness, tmp_path):
    rng = np.random.default_rng(3)
    rec = vr.record(rng, [1])[0]
    rec["n_alt"] = 0  # (format_vcf_line writes nothing for such a record)
    with pytest.raises(RuntimeError, match="exit 2"):
        vr.run(harness, np.zeros((1, 4), np.uint8), np.zeros((1, 4), np.uint8), [vr.line(0, rec)], tmp_dir=tmp_path)


def test_vcf_header_symbols_are_bound_and_exported(lib):
    from basevar_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "basevar_amd_vcf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(bv_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.VCF_EXPORTS) and len(names) == 3
    assert not set(names) & (set(_capi.EXPORTS) | set(_capi.BGZF_EXPORTS))
    for n in names + ["bv_vcf_tile_samples"]:
        assert hasattr(lib, n), n
    assert lib.bv_vcf_tile_samples() % 64 == 0 and lib.bv_vcf_tile_samples() >= 64
    # a null engine is refused, with a message
    for rc in (lib.bv_engine_vcf_format(None, None, None, None), lib.bv_engine_vcf_fetch(None, None, 0, 0, None),
               lib.bv_engine_vcf_deflate(None, None, 0, 0, None, 0, None, None)):
        assert rc == _capi.BV_ERR_INVALID_ARG and b"null engine" in lib.bv_last_error(None)


def test_vcf_struct_layout_matches_header(lib, tmp_path):
    from basevar_amd import _capi
    body = "".join('printf("%s %%zu\\n", offsetof(bv_vcf_lines, %s));\n' % (f, f) for f, _ in _capi.VcfLines._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "basevar_amd_vcf.h"\nint main(void){\n' + body +
                   'printf("sizeof %zu\\n", sizeof(bv_vcf_lines));\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = dict((a, int(b)) for a, b in (l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines()))
    assert vals["sizeof"] == C.sizeof(_capi.VcfLines)
    for f, _ in _capi.VcfLines._fields_:
        assert vals[f] == getattr(_capi.VcfLines, f).offset, f


def test_vcf_kernels_use_no_scratch_and_fit_two_to_a_cu(lib):
    """the code objects' own metadata: no private segment, no spilled register, and LDS for at least two workgroups of the
    write kernel on a CU (160 KiB)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_scratch", os.path.join(ROOT, "tools", "kernel_scratch.py"))
    ks_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks_mod)
    if not os.path.exists(ks_mod.READELF):
        pytest.skip("llvm-readelf not found")
    from basevar_amd import _capi
    ks = [k for k in ks_mod.kernels(_capi.LIB_PATH) if "bv_vcf_" in k["name"]]
    assert len(ks) == 3
    for k in ks:
        assert k["private"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        assert 2 * k["lds"] <= 160 * 1024, k
    write = [k for k in ks if "write" in k["name"]][0]
    assert write["lds"] >= 17 * lib.bv_vcf_tile_samples()  # the image of a tile's output
