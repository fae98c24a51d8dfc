"""CPU tests (no GPU) of the device row writer's definition, basevar_amd/csrc/bv_pileup_text_core.h: the core against the host's
pileup_rows_text inside the stand-alone harness tests/cpp/pileup_text_check.cpp (built with ASan + UBSan and run as a program;
nothing loaded into python runs under a sanitizer), the harness's text against the serial restatement pileup_text_model.rows_text,
both against the reference's own rows under tests/golden/, the new header against the ctypes layer, and the kernels' resources."""
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


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from basevar_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def harness(lib):
    return ptm.build(asan=True)


def test_core_equals_the_host_writer_on_seeded_tiles(harness):
    p = subprocess.run([harness, "random"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and b"FAILS 0" in p.stdout, (p.stdout[-500:], p.stderr[-3000:])
    assert b"PILEUP_TEXT rounds 80 " in p.stdout


SHAPES = [(1, 1, 1.0), (2, 3, 0.5), (63, 2, 0.08), (64, 5, 1.0), (65, 7, 0.5), (70, 40, 0.0), (75, 33, 0.3), (300, 9, 0.08)]


@pytest.mark.parametrize("n,rows,coverage", SHAPES)
def test_model_equals_the_harness(harness, tmp_path, n, rows, coverage):
    t = ptm.random_tile(1000 + n, n, rows, coverage, beg=99990 if n % 2 else 7, pitch_extra=48 if n > 60 else 0, long_tokens=(2, 3, 63, 64, 65, 129, 200))
    text, off = ptm.run_tile(harness, tmp_path, t)
    want, want_off = ptm.rows_text(t)
    assert text == want and (off == want_off).all()
    for first, cnt in ((rows - 1, 1), (0, 0), (rows // 2, rows - rows // 2), (0, 1)):
        part, part_off = ptm.run_tile(harness, tmp_path, t, first, cnt)
        assert part == want[int(want_off[first]):int(want_off[first + cnt])] == ptm.rows_text(t, first, cnt)[0]
        assert (part_off == want_off[first:first + cnt + 1] - want_off[first]).all()


def test_quality_wraps_as_on_the_host(harness, tmp_path):
    """(qual + 33) & 0xFF: 222 gives 0xFF, 223 gives 0, 255 gives 0x20"""
    n = 256
    cell = np.zeros((1, n), np.uint8)
    t = ptm.Tile("c", 1, n, cell, np.arange(n, dtype=np.uint8)[None, :], cell, np.ones((1, n), np.uint16), {}, b"A")
    text, _ = ptm.run_tile(harness, tmp_path, t)
    assert text == ptm.rows_text(t)[0]
    head = b"c\t1\tA\t256\t"  # (the list holds a tab and a line break of its own: it is found by its place)
    assert text.startswith(head + b"0 0 ")
    q = text[len(head) + 4 * n:len(head) + 6 * n - 1]
    assert len(q) == 2 * n - 1 and q[2 * 222] == 0xFF and q[2 * 223] == 0 and q[2 * 255] == 0x20 and q[0] == 33


def test_an_indel_cell_without_a_token_is_named(harness, tmp_path):
    t = ptm.random_tile(5, 70, 6, 0.6)
    key = sorted(t.tokens)[len(t.tokens) // 2]
    del t.tokens[key]
    assert ptm.run_tile(harness, tmp_path, t) == ("missing",) + key
    with pytest.raises(KeyError):
        ptm.rows_text(t)
    first = key[0] - t.beg + 1  # rows behind it: nothing is missing there
    if first < t.rows:
        assert ptm.run_tile(harness, tmp_path, t, first, t.rows - first)[0] == ptm.rows_text(t, first, t.rows - first)[0]


@pytest.mark.parametrize("name", ["w1000", "w65", "w1", "edge"])
def test_corpus_tiles_through_pileup_tile(harness, tmp_path_factory, tmp_path, name):
    """tiles that host/pileup.hpp's pileup_tile makes of the corpus's BAM files (dumped by the pileup harness)"""
    corpus = pr.Corpus(tmp_path_factory.mktemp("ptext_corpus"), 6)
    window = pr.WINDOWS[name]
    d, _ = pr.run_bam(pr.build(asan=True), tmp_path / "d.bin", corpus, 6, window)
    t = ptm.from_dump(d, pr.REF_ID, corpus.fa, window[0])
    text, off = ptm.run_tile(harness, tmp_path, t)
    want, want_off = ptm.rows_text(t)
    assert text == want and (off == want_off).all()
    assert (name != "w1000") or (len(t.tokens) > 5 and max(len(v) for v in t.tokens.values()) > 64)


def test_the_references_own_rows_are_reproduced(harness, tmp_path):
    """tests/golden/reference_pileup_rows.txt.gz holds the reference writer's bytes: parsed back into planes and tokens, the model
    and the core (through a tile file) must give every round again"""
    rounds = ptm.golden_rounds()
    assert len(rounds) == 60
    indels = 0
    for r, want in rounds:
        t = ptm.parse_rows(want)
        indels += len(t.tokens)
        assert ptm.rows_text(t)[0] == want, r
        assert ptm.run_tile(harness, tmp_path, t)[0] == want, r
    assert indels > 500


# ---------------------------------------------------------------------------------------------------------- the header and the kernels
def test_pileup_text_header_symbols_are_bound_and_exported(lib):
    from basevar_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "basevar_amd_pileup_text.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(bv_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.PILEUP_TEXT_EXPORTS) and len(names) == 4
    assert not set(names) & (set(_capi.EXPORTS) | set(_capi.BGZF_EXPORTS) | set(_capi.VCF_EXPORTS) | set(_capi.PILEUP_EXPORTS))
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bv_pileup_text_tile_samples() % 64 == 0
    for rc in (lib.bv_engine_pileup_text(None, None, None, None), lib.bv_engine_pileup_text_fetch(None, None, 0, 0, None),
               lib.bv_engine_pileup_text_deflate(None, None, 0, 0, None, 0, None, None)):
        assert rc == _capi.BV_ERR_INVALID_ARG and b"null engine" in lib.bv_last_error(None)


def test_pileup_text_struct_layout_matches_header(lib, tmp_path):
    from basevar_amd import _capi
    structs = [("bv_pileup_tile", _capi.PileupTile), ("bv_pileup_text", _capi.PileupText)]
    body = "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (n, f, n, f) for n, t in structs for f, _ in t._fields_)
    body += "".join('printf("%s.sizeof %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in structs)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "basevar_amd_pileup_text.h"\nint main(void){\n' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = dict((a, int(b)) for a, b in (l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines()))
    for n, t in structs:
        assert vals[n + ".sizeof"] == C.sizeof(t)
        for f, _ in t._fields_:
            assert vals["%s.%s" % (n, f)] == getattr(t, f).offset, (n, f)
    assert ptm.TOKEN_DTYPE == _capi.PILEUP_TOKEN_DTYPE


def test_pileup_text_kernels_use_no_scratch_no_spills_and_little_lds(lib):
    """the code objects' own metadata: no private segment, no spilled register, LDS small enough for two workgroups a CU and more"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_scratch", os.path.join(ROOT, "tools", "kernel_scratch.py"))
    ks_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks_mod)
    if not os.path.exists(ks_mod.READELF):
        pytest.skip("llvm-readelf not found")
    from basevar_amd import _capi
    ks = [k for k in ks_mod.kernels(_capi.LIB_PATH) if "bv_ptext_" in k["name"]]
    assert len(ks) == 3  # count, scan, write
    for k in ks:
        assert k["private"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        assert 2 * k["lds"] <= 160 * 1024 and k["lds"] <= 16 * 1024, k
