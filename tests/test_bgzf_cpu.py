"""CPU tests (no GPU) of the device BGZF path: the new public header against the ctypes layer and the library, the CPU build of
the DEFLATE decoder's core (basevar_amd/csrc/bv_inflate_core.h, the code the kernel compiles) against zlib over the whole
valid and damaged corpus of tests/bgzf_corpus.py, plain and under ASan + UBSan, and the inflate kernel's resources."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzf_corpus as bc  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from basevar_amd import _capi
    return _capi.load()


def test_bgzf_header_symbols_are_bound_and_exported(lib):
    from basevar_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "basevar_amd_bgzf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(bv_[a-z0-9_]+)\s*\(", hdr)))
    assert names and sorted(_capi.BGZF_EXPORTS) == names
    assert not set(names) & set(_capi.EXPORTS)
    for n in names:
        assert hasattr(lib, n), n
    assert re.search(r"#define\s+BV_ERR_DATA\s+\(-6\)", hdr) and _capi.BV_ERR_DATA == -6


def test_bgzf_struct_layout_matches_header(tmp_path):
    from basevar_amd import _capi
    structs = (("bv_bgzf_members", _capi.BgzfMembers), ("bv_bgzf_rows", _capi.BgzfRows), ("bv_bgzf_cursor", _capi.BgzfCursor))
    body = "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (n, f, n, f) for n, c in structs for f, _ in c._fields_)
    body += "".join('printf("sizeof.%s %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in structs)
    body += "".join('printf("%s %%d\\n", (int)%s);\n' % (k, k) for k in ("BV_BGZF_OK", "BV_BGZF_BAD_HEADER", "BV_BGZF_BAD_DEFLATE", "BV_BGZF_BAD_SIZE",
                                                                          "BV_BGZF_BAD_CRC", "BV_ERR_DATA"))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "basevar_amd_bgzf.h"\nint main(void){\n'
                   + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = dict((a, int(b)) for a, b in (l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines()))
    for n, c in structs:
        assert vals["sizeof." + n] == C.sizeof(c), n
        for f, _ in c._fields_:
            assert vals[n + "." + f] == getattr(c, f).offset, (n, f)
    for k in ("BV_BGZF_OK", "BV_BGZF_BAD_HEADER", "BV_BGZF_BAD_DEFLATE", "BV_BGZF_BAD_SIZE", "BV_BGZF_BAD_CRC", "BV_ERR_DATA"):
        assert vals[k] == getattr(_capi, k), k
    assert (bc.OK, bc.BAD_HEADER, bc.BAD_DEFLATE, bc.BAD_SIZE, bc.BAD_CRC) == (0, 1, 2, 3, 4)


def test_bgzf_calls_refuse_a_null_engine(lib):
    from basevar_amd import _capi
    assert lib.bv_engine_bgzf_inflate(None, None, None, 0, _capi.BV_MEM_HOST, None, None, None) == _capi.BV_ERR_INVALID_ARG
    assert b"bv_engine_bgzf_inflate: null engine" in lib.bv_last_error(None)
    assert lib.bv_engine_text_parse_bgzf(None, None, None, 0, None, None, None, None) == _capi.BV_ERR_INVALID_ARG
    assert b"bv_engine_text_parse_bgzf: null engine" in lib.bv_last_error(None)
    assert lib.bv_engine_text_rows_fetch(None, None, 0, None, None, None) == _capi.BV_ERR_INVALID_ARG
    assert b"bv_engine_text_rows_fetch: null engine" in lib.bv_last_error(None)


@pytest.fixture(scope="module")
def corpus():
    valid = bc.valid_corpus()
    damaged = bc.damaged_corpus()
    assert len(valid) > 100 and len(damaged) > 300
    return valid, damaged


def _check(exe, corpus, tmp_path):
    valid, damaged = corpus
    p, rows = bc.core_verdicts(exe, [m for _, m, _ in valid], tmp_path)
    report = [l for l in p.stderr.splitlines() if "Sanitizer" in l or "runtime error:" in l]
    assert not report and p.returncode == 0, p.stderr[-3000:]
    assert len(rows) == len(valid)
    wrong = [(n, r) for (n, _, d), r in zip(valid, rows) if r[0] != bc.OK or r[1] != bc.OK or r[3] != len(d)]
    assert not wrong, wrong[:10]
    mixed = bc.assert_block_coverage([n for n, _, _ in valid], [m for _, m, _ in valid], rows)
    p, rows = bc.core_verdicts(exe, [m for _, m in damaged], tmp_path)
    print(p.stderr[-2000:])  # (members that zlib and the core name differently are listed there; OK against not OK is what is held)
    report = [l for l in p.stderr.splitlines() if "Sanitizer" in l or "runtime error:" in l]
    assert not report and p.returncode == 0, p.stderr[-3000:]
    assert len(rows) == len(damaged)
    seen = {r[0] for r in rows}
    assert seen == {bc.OK, bc.BAD_HEADER, bc.BAD_DEFLATE, bc.BAD_SIZE, bc.BAD_CRC}, seen  # every status occurs
    by_name = {n: r[0] for (n, _), r in zip(damaged, rows)}
    for n, want in (("distance_too_far", bc.BAD_DEFLATE), ("btype3", bc.BAD_DEFLATE), ("stored_len_nlen", bc.BAD_DEFLATE), ("cl_oversubscribed", bc.BAD_DEFLATE),
                    ("cl_incomplete", bc.BAD_DEFLATE), ("lit_oversubscribed", bc.BAD_DEFLATE), ("lit_incomplete", bc.BAD_DEFLATE),
                    ("no_end_of_block_code", bc.BAD_DEFLATE), ("fixed_symbol_286", bc.BAD_DEFLATE), ("fixed_distance_30", bc.BAD_DEFLATE),
                    ("hlit_287", bc.BAD_DEFLATE), ("hdist_31", bc.BAD_DEFLATE), ("only_end_of_block", bc.OK), ("no_distance_codes", bc.OK),
                    ("stored_ok", bc.OK), ("distance_ok", bc.OK), ("rows/l6/default/isize+1", bc.BAD_SIZE), ("rows/l6/default/isize-1", bc.BAD_SIZE),
                    ("rows/l6/default/crc", bc.BAD_CRC), ("rows/l6/default/bsize+1", bc.BAD_HEADER), ("rows/l6/default/cut5", bc.BAD_SIZE),
                    ("rows_short/l0/nlen", bc.BAD_DEFLATE), ("rows/l1/default/isize_huge", bc.BAD_SIZE)):
        assert by_name[n] == want, (n, by_name[n], want)
    return mixed


def test_inflate_core_against_zlib(corpus, tmp_path):
    """zlib judges every member of the valid and of the damaged corpus; the core agrees on OK / not OK everywhere, gives zlib's
    bytes, leaves the guard bytes alone; the valid corpus holds all three block types and members that mix them"""
    mixed = _check(bc.build_core_check(tmp_path), corpus, tmp_path)
    assert len(mixed) >= 3


def test_inflate_core_under_asan_and_ubsan(corpus, tmp_path):
    """the same run with the `sanitize` build of basevar_amd/csrc/Makefile: no report over either corpus"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "basevar_amd", "csrc"), "../lib/san/inflate_core_check.asan"])
    _check(os.path.join(ROOT, "basevar_amd", "lib", "san", "inflate_core_check.asan"), corpus, tmp_path)


def test_new_sources_hold_no_scalar_store_mnemonics():
    """the new sources hold none of the scalar-store / scalar-cache-writeback mnemonics"""
    words = ["s_" + w for w in ("store_dword", "buffer_store_", "scratch_store_", "atomic_", "buffer_atomic_", "dcache_wb", "dcache_discard")]
    for f in ("basevar_amd/csrc/bv_inflate.hip", "basevar_amd/csrc/bv_inflate_core.h", "basevar_amd/csrc/bv_text.hip", "tests/cpp/inflate_core_check.cpp",
              "tests/cpp/producer_raw_check.cpp", "include/basevar_amd_bgzf.h", "basevar_amd/host/batch_producer.hpp", "basevar_amd/host/bv_call.cpp"):
        txt = open(os.path.join(ROOT, f)).read().lower()
        assert not [w for w in words if w in txt], f


def test_inflate_kernel_resources(lib):
    """The inflate kernel keeps its window and tables in at most 160 KiB of LDS (two workgroups per CU need <= 80 KiB) and owns
    no scratch memory (the code object's own metadata, read with the toolchain's llvm-readelf that built it)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_scratch", os.path.join(ROOT, "tools", "kernel_scratch.py"))
    ks_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks_mod)
    assert os.path.exists(ks_mod.READELF), "llvm-readelf of the ROCm toolchain not found"
    from basevar_amd import _capi
    ks = [k for k in ks_mod.kernels(_capi.LIB_PATH) if "bv_bgzf_inflate_kernel" in k["name"]]
    assert len(ks) == 1, ks
    k = ks[0]
    assert 64 * 1024 <= k["lds"] <= 80 * 1024, k
    assert k["private"] == 0 and k["vgpr_spill"] == 0, k


def _bgzf_file(path, data, member):
    with open(path, "wb") as fh:
        for at in range(0, len(data), member):
            fh.write(bc.member(data[at:at + member], 1 if member < 1000 else 6))
        fh.write(bc.member(b""))


def test_raw_reader_reproduces_the_text_mode_rows(tmp_path):
    """tests/cpp/producer_raw_check.cpp: BgzfRawReader's runs, inflated and cut into lines by a CPU stand-in for the device under
    the contract of bv_engine_text_parse_bgzf, give run_text's rows, row for row, over whole files -- written here with another
    member size per file, another number of header lines, a last line without its line break, and rewritten by BgzfWriter --
    for several run sizes and max_positions, 1 among them."""
    import numpy as np
    rng = np.random.default_rng(41)
    n_pos, files = 700, []
    for f, (samples, member, headers) in enumerate(((3, 0x100, 2), (40, 0x1000, 5), (200, 0xff00, 3), (7, 333, 4))):
        ids = ",".join("s%d_%d" % (f, k) for k in range(samples))
        head = ["##fileformat=BaseVarBatchFile_v1.0", "##SampleIDs=" + ids] + ["##extra header line %d" % k for k in range(headers - 3)] + \
               ["#CHROM\tPOS\tREF\tDepth\tMappingQuality\tReadbases\tReadbasesQuality\tReadPositionRank\tStrand"]
        rows = []
        for p in range(n_pos):
            cov = rng.random(samples) < 0.3
            col = lambda a, b: " ".join(a[int(rng.integers(0, len(a)))] if c else b for c in cov)  # noqa: E731
            rows.append("chr7\t%d\tG\t%d\t%s\t%s\t%s\t%s\t%s" % (5000 + p, int(cov.sum()), col(["60", "37", "0"], "0"), col(["A", "C", "G", "T", "+AT"], "N"),
                                                                col(["I", "5", "#"], "!"), col(["12", "150", "7"], "0"), col(["+", "-"], ".")))
        data = ("\n".join(head + rows) + ("\n" if f % 2 else "")).encode()  # files 0 and 2 end without a line break
        path = str(tmp_path / ("batch_%d.gz" % f))
        _bgzf_file(path, data, member)
        files.append(path)
    exe = str(tmp_path / "producer_raw_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "producer_raw_check.cpp"), "-lz", "-o", exe])
    (tmp_path / "rw").mkdir()
    p = subprocess.run([exe, ",".join(files), str(tmp_path / "rw")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and p.stdout.count("OK ") == 2 and "FAIL" not in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "%d rows of 4 files" % (n_pos * 4) in p.stdout
