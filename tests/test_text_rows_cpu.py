"""CPU tests (no GPU) of the batchfile text-row entry points (bv_engine_text_parse / bv_engine_text_submit,
include/basevar_amd.h): the header declares them, the library exports them, the ctypes struct has the header's layout,
and calls without an engine are refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from basevar_amd import _capi
    return _capi.load()


def test_header_declares_the_text_row_calls():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "basevar_amd.h")).read(), flags=re.S)
    m = re.search(r"int\s+bv_engine_text_parse\s*\(([^)]*)\)\s*;", hdr)
    assert m and [p.strip() for p in m.group(1).split(",")] == [
        "bv_engine *e", "const bv_text_rows *rows", "const uint8_t *group_id", "uint32_t n_groups", "uint8_t *row_state", "void *stream"]
    m = re.search(r"int\s+bv_engine_text_submit\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 9
    from basevar_amd import _capi
    assert {"bv_engine_text_parse", "bv_engine_text_submit"} <= set(_capi.EXPORTS)


def test_text_rows_layout_matches_header(tmp_path):
    from basevar_amd import _capi
    src = tmp_path / "layout.c"
    names = [f[0] for f in _capi.TextRows._fields_]
    body = "".join('printf("%s %%zu\\n", offsetof(bv_text_rows, %s));\n' % (n, n) for n in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "basevar_amd.h"\nint main(void){\nprintf("size %zu\\n", sizeof(bv_text_rows));\n'
                   'printf("skip %d host %d indel %d\\n", BV_TEXT_SKIP, BV_TEXT_HOST, BV_TEXT_INDEL);\n' + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.split(" ", 1) for l in subprocess.check_output([str(exe)]).decode().strip().split("\n"))
    assert int(out["size"]) == C.sizeof(_capi.TextRows)
    for n in names:
        assert int(out[n]) == getattr(_capi.TextRows, n).offset, n
    assert out["skip"] == "%d host %d indel %d" % (_capi.BV_TEXT_SKIP, _capi.BV_TEXT_HOST, _capi.BV_TEXT_INDEL)


def test_calls_without_an_engine_are_refused(lib):
    from basevar_amd import _capi
    text = b"chr1\t5\tA\t1\t60\tA\tI\t3\t+\n"
    off = (C.c_uint64 * 2)(0, len(text))
    fs = (C.c_uint32 * 1)(1)
    rows = _capi.TextRows(C.cast(C.c_char_p(text), C.c_void_p), C.cast(off, C.c_void_p), C.cast(fs, C.c_void_p), len(text), 1, 1, 0)
    state = (C.c_uint8 * 1)()
    assert lib.bv_engine_text_parse(None, C.byref(rows), None, 0, state, None) == _capi.BV_ERR_INVALID_ARG
    assert b"null engine" in lib.bv_last_error(None)
    assert lib.bv_engine_text_parse(None, None, None, 0, state, None) == _capi.BV_ERR_INVALID_ARG
    out = (C.c_uint8 * 208)()
    assert lib.bv_engine_text_submit(None, state, None, 1, out, None, None, None, None) == _capi.BV_ERR_INVALID_ARG


def test_producer_text_mode_hands_on_the_plain_loops_lines(tmp_path):
    """BatchfileProducer::run_text (the rows packed for the device parser) on BGZF, gzip and plain batchfiles, on files of
    uneven sample counts and on a file that ends early: every position's lines, in order, on 1 / 2 / 3 / 8 threads and three
    block sizes -- built once with AddressSanitizer + UBSan and once with ThreadSanitizer"""
    from test_host_formats import _write_batchfiles, make_batchfiles
    from test_sanitize_cpu import run
    sets = []
    d = tmp_path / "a"; d.mkdir()
    sets.append(_write_batchfiles(str(d), 5, 37, 700, seed=1, plain_last=True))
    d = tmp_path / "b"; d.mkdir()
    sets.append(_write_batchfiles(str(d), 4, 50, [300, 300, 171, 300], seed=2))
    sets.append(make_batchfiles(tmp_path, n_sites=200, n_samples=60)[0])
    uneven = []
    for k, (per, seed) in enumerate(((3, 31), (41, 32), (200, 33))):
        d = tmp_path / ("u%d" % k); d.mkdir()
        uneven += _write_batchfiles(str(d), 1, per, 150, seed=seed)
    sets.append(uneven)
    src = os.path.join(ROOT, "tests", "cpp", "producer_text_check.cpp")
    for kind, flags in (("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), ("tsan", ["-fsanitize=thread"])):
        exe = str(tmp_path / ("ptc." + kind))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-pthread", "-I",
                               os.path.join(ROOT, "include")] + flags + [src, "-lz", "-o", exe])
        for files in sets:
            p = run([exe, ",".join(files)])
            assert p.returncode == 0 and p.stdout.startswith("OK "), p.stdout + p.stderr
