"""CPU tests (no GPU) of the device's number formats and record lines: basevar_amd/csrc/bv_numfmt_core.h against snprintf and
basevar_amd/csrc/bv_record_text_core.h -- the code the kernels of bv_record_text.hip compile -- against host/vcf_emit.hpp's
format_vcf_head and format_cvg_line, inside the stand-alone harness tests/cpp/record_text_check.cpp built with ASan + UBSan and
run as a program; the serial Python model tests/record_text_model.py against the harness's dump; the header against the ctypes
layer; and the kernels' resources."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import record_text_model as model  # noqa: E402
import record_text_ref as ref  # noqa: E402
from basevar_amd import _capi  # noqa: E402

GROUP_COUNTS = [0, 1, 2, 40, 255]


@pytest.fixture(scope="module")
def exe():
    return ref.build(asan=True)


def names_of(n_groups):
    return [(b"G%d" % j) * (1 + j % 3) for j in range(n_groups)]


def hold_model(lines, names, dump):
    """The model's predicate is the harness's for every line, and its two lines are the host formatters' for every line the
    predicate accepts: none of those is skipped."""
    held = 0
    for k, (ln, (on, gt, vcf, cvg, indel)) in enumerate(zip(lines, dump)):
        groups = ln["groups"] if names else ()
        assert model.on_device(ln["rec"], groups) == on, k
        assert model.indel_column(ln["tokens"]) == indel, k
        assert model.gt_codes(ln["rec"], ln["ref"]) == gt, k
        if not on:
            continue
        assert model.vcf_head(ln["rec"], groups, names, ln["chrom"], ln["pos"], ln["ref"]) == vcf, k
        assert model.cvg_row(ln["rec"], ln["chrom"], ln["pos"], ln["ref"], b"" if indel == b"." else indel) == cvg, k
        held += 1
    return held


def test_numbers_against_snprintf(exe):
    """Ties, carries, the %g notation switch, both ends of each domain, zeros, denormals, NaN and inf, and 2 x 10^7 seeded doubles"""
    out = ref.run_numbers(exe)
    m = re.search(r"formatted: %f (\d+), %g (\d+), \(int\) (\d+); outside %g's domain (\d+); of the scaled \[0, 1\) set (\d+) of (\d+)", out)
    assert m, out
    n_f6, n_g6, n_iod, _, scaled, of = (int(x) for x in m.groups())
    assert of >= 10 ** 7 and scaled * 10 >= of * 9
    assert n_f6 >= 10 ** 7 and n_g6 >= 10 ** 7 and n_iod >= 10 ** 7


@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
def test_seeded_lines(exe, tmp_path, n_groups):
    names = names_of(n_groups)
    lines = ref.seeded_lines(100 + n_groups, 240 if n_groups < 40 else 60, n_groups)
    dump = ref.run_lines(exe, lines, names, tmp_path)
    assert hold_model(lines, names, dump) == len(lines)  # every seeded record is in the domain
    assert any(vcf == b"" for _, _, vcf, _, _ in dump) and any(cvg == b"" for _, _, _, cvg, _ in dump)
    assert any(indel != b"." for *_, indel in dump) and any(b"LowQual" in vcf for _, _, vcf, _, _ in dump)


def test_special_values_in_every_field(exe, tmp_path):
    names = names_of(2)
    lines = ref.special_lines(2)
    dump = ref.run_lines(exe, lines, names, tmp_path)
    held = hold_model(lines, names, dump)
    n_special = len(ref.SPECIAL) * (len(ref.F6_FIELDS) + len(ref.IOD_FIELDS) + 4)
    assert all(on for on, *_ in dump[:n_special]) and held >= n_special
    assert sum(1 for on, *_ in dump[n_special:] if not on) >= 4 * len(ref.OUTSIDE)


def golden_records():
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")) + glob.glob(os.path.join(ROOT, "tests", "golden", "reference_fresh", "*.npz"))):
        z = np.load(path)
        if "expected_sites" not in z.files:
            continue
        sites = np.frombuffer(z["expected_sites"].tobytes(), dtype=_capi.SITE_DTYPE)
        groups = None
        if "expected_groups" in z.files and z["expected_groups"].size:
            groups = np.frombuffer(z["expected_groups"].tobytes(), dtype=_capi.GROUP_DTYPE).reshape(len(sites), -1)
        ref_base = z["ref_base"] if "ref_base" in z.files else np.zeros(len(sites), np.uint8)
        yield os.path.basename(path), sites, groups, ref_base


def test_golden_records(exe, tmp_path):
    """The records of every golden file: the model against the host formatters, no record skipped that the predicate accepts"""
    total = held = 0
    for name, sites, groups, ref_base in golden_records():
        G = 0 if groups is None else groups.shape[1]
        names = names_of(G)
        lines = [ref.line(sites[k], groups[k] if G else None, chrom=b"chr22", pos=10000 + k, ref=b"ACGTN"[int(ref_base[k]) % 5:int(ref_base[k]) % 5 + 1]
                          if int(ref_base[k]) < 5 else bytes([int(ref_base[k])])) for k in range(len(sites)) if int(sites[k]["n_alt"]) <= 4]
        dump = ref.run_lines(exe, lines, names, tmp_path)
        held += hold_model(lines, names, dump)
        total += len(lines)
    assert total > 1000 and held > total // 2, (total, held)


def test_predicate_through_the_abi():
    from basevar_amd import BaseTypeEngine
    lines = ref.special_lines(2)
    sites = np.array([ln["rec"] for ln in lines], dtype=_capi.SITE_DTYPE)
    groups = np.array([ln["groups"] for ln in lines], dtype=_capi.GROUP_DTYPE)
    got = BaseTypeEngine.record_text_on_device(sites, groups)
    want = np.array([model.on_device(ln["rec"], ln["groups"]) for ln in lines])
    assert (got == want).all() and want.any() and not want.all()
    nan = sites[0].copy()
    nan["af"][0] = np.nan  # the Q0 site of SURVEY section 8a
    assert not BaseTypeEngine.record_text_on_device(nan.reshape(1))[0]


def test_header_matches_ctypes():
    """include/basevar_amd_record_text.h: its exports are the library's, its struct is _capi's"""
    text = open(os.path.join(ROOT, "include", "basevar_amd_record_text.h")).read()
    declared = sorted(set(re.findall(r"^int (bv_\w+)\(", text, re.M)))
    assert declared == sorted(_capi.RECORD_TEXT_EXPORTS)
    lib = _capi.load()
    for name in declared:
        assert hasattr(lib, name), name
    body = re.search(r"typedef struct bv_record_lines \{(.*?)\} bv_record_lines;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip() for f in decl.strip().split(" ", 2 if decl.strip().startswith("const") else 1)[-1].split(",")]
    assert fields == [f for f, _ in _capi.RecordLines._fields_]
    assert C.sizeof(_capi.RecordLines) == 13 * 8 + 5 * 4 + 4  # thirteen pointers, five 32-bit words, padding
    assert _capi.RECORD_TEXT_NAME_MAX == int(re.search(r"BV_RECORD_TEXT_NAME_MAX (\d+)u", text).group(1))
    assert _capi.RECORD_TEXT_INDEL_MAX == int(re.search(r"BV_RECORD_TEXT_INDEL_MAX (\d+)u", text).group(1))


def test_kernels_use_no_scratch():
    """The compiler's resource summary of bv_record_text.hip: no scratch, no spilled register, the LDS image of DESIGN section 6"""
    src = os.path.join(ROOT, "basevar_amd", "csrc", "bv_record_text.hip")
    p = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    kernels = re.findall(r"Function Name: (\S+)", out)
    assert len(kernels) == 2 and any("count" in k for k in kernels) and any("write" in k for k in kernels)
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)] == [0, 0]
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out)] == [0, 0] and [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", out)] == [0, 0]
    assert max(int(x) for x in re.findall(r" VGPRs: (\d+)", out)) <= 128
    assert sorted(int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out)) == [0, 16 + 64 * 272 + 16]
    text = open(src).read() + open(os.path.join(ROOT, "basevar_amd", "csrc", "bv_record_text_core.h")).read() + open(os.path.join(ROOT, "basevar_amd", "csrc", "bv_numfmt_core.h")).read()
    assert "atomic" not in text.replace("No atomics", "") and "printf" not in text.replace("No printf", "").replace("snprintf", "").replace("nor `printf`", "")
