"""CPU tests (no GPU) of the definition of the rows of a sample part ("ROWS OF A PART", basevar_amd/csrc/bv_pileup_text_core.h): the
core's bv_ptext_row_part against the host's pileup_rows_text on a PileupTile sliced to the part's columns, with token samples
rebased, inside the stand-alone harness tests/cpp/pileup_text_parts_check.cpp (built with ASan + UBSan and run as a program;
nothing loaded into python runs under a sanitizer); the harness's text against pileup_text_parts_model.parts_text; the new header
against the ctypes layer; and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pileup_ref as pr  # noqa: E402
import pileup_text_model as ptm  # noqa: E402
import pileup_text_parts_model as ppm  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from basevar_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def harness(lib):
    return ppm.build(asan=True)


def test_core_parts_equal_the_host_writer_on_sliced_seeded_tiles(harness):
    p = subprocess.run([harness, "random"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and b"FAILS 0" in p.stdout, (p.stdout[-500:], p.stderr[-3000:])
    assert b"PILEUP_TEXT_PARTS rounds 80 " in p.stdout


# (n, rows, coverage, part_first): one part of all; single samples; B-sized parts with a remainder; gaps before and behind
SHAPES = [(1, 1, 1.0, [0, 1]), (2, 3, 0.5, [0, 1, 2]), (65, 7, 0.5, [0, 65]), (65, 5, 1.0, [1, 64]), (70, 9, 0.0, [0, 7, 14, 70]),
          (75, 33, 0.3, [3, 10, 17, 24, 31, 74]), (300, 9, 0.08, [0, 200, 300]), (300, 4, 0.5, [8, 9, 23, 208, 299])]


@pytest.mark.parametrize("n,rows,coverage,part_first", SHAPES)
def test_model_equals_the_harness(harness, tmp_path, n, rows, coverage, part_first):
    t = ptm.random_tile(2000 + n + rows, n, rows, coverage, beg=99990 if n % 2 else 7, pitch_extra=48 if n > 60 else 0, long_tokens=(2, 3, 63, 64, 65, 129, 200))
    text, off = ppm.run_parts(harness, tmp_path, t, part_first)
    want, want_off = ppm.parts_text(t, part_first)
    assert text == want and (off == want_off).all() and off.size == (len(part_first) - 1) * rows + 1
    if part_first == [0, n]:
        assert text == ptm.rows_text(t)[0]
    for first, cnt in ((rows - 1, 1), (0, 0), (rows // 2, rows - rows // 2)):
        sub, sub_off = ppm.run_parts(harness, tmp_path, t, part_first, first, cnt)
        want, want_off = ppm.parts_text(t, part_first, first, cnt)
        assert sub == want and (sub_off == want_off).all()


def test_depth_and_lists_are_the_parts_own(harness, tmp_path):
    """a row whose claimed cells all lie outside the part: Depth 0, all placeholders; the neighbour part has them"""
    t = ptm.random_tile(9, 40, 2, 1.0, indel_frac=0.0)
    t.rank[0, 10:30] = 0
    text, off = ppm.run_parts(harness, tmp_path, t, [10, 30, 40])
    row = text[:int(off[1])].split(b"\t")
    assert row[3] == b"0" and row[4] == b" ".join([b"0"] * 20) and row[8] == b" ".join([b"."] * 20) + b"\n"
    assert text[int(off[2]):int(off[3])].split(b"\t")[3] == b"10"


def test_a_missing_token_is_named_by_its_absolute_sample_and_ignored_in_a_gap(harness, tmp_path):
    t = ptm.random_tile(5, 70, 6, 0.6)
    key = sorted(t.tokens)[len(t.tokens) // 2]
    del t.tokens[key]
    s = key[1]
    inside = [max(s - 3, 0), s + 1] if s else [0, 5]
    assert ppm.run_parts(harness, tmp_path, t, inside) == ("missing",) + key
    with pytest.raises(KeyError) as ei:
        ppm.parts_text(t, inside)
    assert ei.value.args[0] == key
    for gap in ([0, s] if s else None, [s + 1, 70] if s + 1 < 70 else None):
        if gap:
            assert ppm.run_parts(harness, tmp_path, t, gap)[0] == ppm.parts_text(t, gap)[0]


@pytest.mark.parametrize("name", ["w1000", "w65", "w1", "edge"])
def test_corpus_tiles_through_pileup_tile(harness, tmp_path_factory, tmp_path, name):
    """tiles that host/pileup.hpp's pileup_tile makes of the corpus's BAM files (dumped by the pileup harness), cut into parts"""
    corpus = pr.Corpus(tmp_path_factory.mktemp("pparts_corpus"), 6)
    window = pr.WINDOWS[name]
    d, _ = pr.run_bam(pr.build(asan=True), tmp_path / "d.bin", corpus, 6, window)
    t = ptm.from_dump(d, pr.REF_ID, corpus.fa, window[0])
    for part_first in ([0, 6], [0, 1, 2, 3, 4, 5, 6], [0, 4, 6], [1, 3, 5]):
        text, off = ppm.run_parts(harness, tmp_path, t, part_first)
        want, want_off = ppm.parts_text(t, part_first)
        assert text == want and (off == want_off).all()


# ---------------------------------------------------------------------------------------------------------- the header and the kernels
def test_parts_header_symbols_are_bound_and_exported(lib):
    from basevar_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "basevar_amd_pileup_text_parts.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(bv_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.PILEUP_TEXT_PARTS_EXPORTS) == ["bv_engine_pileup_text_parts"]
    assert not set(names) & (set(_capi.EXPORTS) | set(_capi.BGZF_EXPORTS) | set(_capi.VCF_EXPORTS) | set(_capi.PILEUP_EXPORTS) | set(_capi.PILEUP_TEXT_EXPORTS))
    assert hasattr(lib, names[0])
    assert lib.bv_engine_pileup_text_parts(None, None, None, None) == _capi.BV_ERR_INVALID_ARG and b"null engine" in lib.bv_last_error(None)
    # the header that the calls continue declares them too
    assert '#include "basevar_amd_pileup_text_parts.h"' in open(os.path.join(ROOT, "include", "basevar_amd_pileup_text.h")).read()


def test_parts_struct_layout_matches_header(lib, tmp_path):
    from basevar_amd import _capi
    n, t = "bv_pileup_text_parts", _capi.PileupTextParts
    body = "".join('printf("%s %%zu\\n", offsetof(%s, %s));\n' % (f, n, f) for f, _ in t._fields_) + 'printf("sizeof %%zu\\n", sizeof(%s));\n' % n
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "basevar_amd_pileup_text.h"\nint main(void){\n' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = dict((a, int(b)) for a, b in (l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines()))
    assert vals["sizeof"] == C.sizeof(t)
    for f, _ in t._fields_:
        assert vals[f] == getattr(t, f).offset, f


def test_parts_kernels_use_no_scratch_no_spills_and_little_lds(lib):
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_scratch", os.path.join(ROOT, "tools", "kernel_scratch.py"))
    ks_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks_mod)
    if not os.path.exists(ks_mod.READELF):
        pytest.skip("llvm-readelf not found")
    from basevar_amd import _capi
    ks = [k for k in ks_mod.kernels(_capi.LIB_PATH) if "bv_pparts_" in k["name"]]
    assert len(ks) == 3  # count, scan, write
    for k in ks:
        assert k["private"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        assert 2 * k["lds"] <= 160 * 1024 and k["lds"] <= 16 * 1024, k
