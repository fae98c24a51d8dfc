"""CPU tests (no GPU) of the device BGZF path: the new public header against the ctypes layer and the library, the CPU build of
the DEFLATE decoder's core (basevar_amd/csrc/bv_inflate_core.h, the code the kernel compiles) against zlib over the whole
valid and damaged corpus of tests/bgzf_corpus.py and over its foreign corpus (streams zlib's compressor never writes; the tracer
of tests/deflate_writer.py says what each holds), plain and under ASan + UBSan, and the inflate kernel's resources."""
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


@pytest.fixture(scope="module")
def foreign():
    valid = bc.foreign_corpus()
    damaged = bc.foreign_damaged()
    assert len(valid) > 80 and len(damaged) > 30
    assert len({n for n, _, _ in valid}) == len(valid) and len({n for n, _ in damaged}) == len(damaged)
    return valid, damaged


def test_tracer_gives_zlibs_bytes_and_the_foreign_corpus_holds_every_feature(foreign):
    """tests/deflate_writer.py's tracer inflates every valid foreign member to zlib's bytes (raw inflate of the payload, and gzip
    inflate of the whole member: the wrapper's judge), and the features it counts there are all of bc.required_features();
    one member is everything at once."""
    import zlib
    valid, _ = foreign
    total, per = bc.foreign_features(valid)  # (asserts the tracer's text against zlib's, member by member)
    for name, m, d in valid:  # (gzip expects CRC32 and ISIZE right behind the final block; BGZF finds them by the BC length)
        assert per[name]["trailing_bytes"] or zlib.decompress(m, 31) == d, name
    assert sum(1 for n in per if per[n]["trailing_bytes"]) == 1
    bc.assert_features_hit(total)
    assert per["everything_at_once"]["everything_at_once"] == 1 and per["everything_at_once"]["cl_len7"]
    assert len(bc.payload_of(dict((n, m) for n, m, _ in valid)["everything_at_once"])) < 40000


def test_zlibs_own_streams_lack_what_the_foreign_corpus_adds(corpus):
    """The tracer over all of valid_corpus() (every member; zlib's bytes again): none of the features of bc.ABSENT_FROM_ZLIB
    occurs there, the text sizes mod 16 are 0, 1, 8 and 12 and below 16 bytes 0 and 1.  (If a zlib build does write one of
    them, the assertion names it; it may then be dropped from that list alone.)"""
    valid, _ = corpus
    total, _ = bc.foreign_features(valid)
    assert not [k for k in bc.ABSENT_FROM_ZLIB if total[k]]
    assert not [k for k in total if k.startswith("dist_bits:") and int(k[10:]) > 11] and not total["hclen:19"]
    assert {len(d) % 16 for _, _, d in valid} == {0, 1, 8, 12} and {len(d) for _, _, d in valid if len(d) < 16} == {0, 1}
    added = [k for k in bc.required_features() if not total[k]]
    assert len(added) > 100, len(added)


def test_writer_against_itself(foreign):
    """expand() of the tokens the writer was given is what zlib inflates from what it wrote, for every valid foreign member;
    transcode() keeps the text and writes the codes it was asked for"""
    import zlib
    import deflate_writer as dw
    valid, _ = foreign
    blocks = bc.foreign_blocks()
    for name, _, d in valid:
        assert dw.block_text(blocks[name]) == d, name
    for n in (16, 30, 286):
        lens = dw.skewed_lengths(n, 15)
        assert len(lens) == n and dw.kraft(lens) == 1 << 15 and set(lens) == set(range(lens[0], 16)), n
    assert dw.skewed_lengths(16, 15) == list(range(1, 16)) + [15]
    text = valid[0][2] * 3 + bytes(range(256)) * 40
    payload, out = dw.transcode(bc.deflate(text, 6), cut=40, stored_every=3)
    assert out == text and zlib.decompress(payload, -15) == text
    f = dw.trace(payload).features
    assert f["hclen:19"] and f["hclen19_slot18_nonzero"] and f["hlit:286"] and f["hdist:30"] and f["blocks:0"] and f["blocks:2"] > 2


def _check_foreign(exe, foreign, tmp_path):
    import zlib
    valid, damaged = foreign
    p, rows = bc.core_verdicts(exe, [m for _, m, _ in valid], tmp_path)
    report = [l for l in p.stderr.splitlines() if "Sanitizer" in l or "runtime error:" in l]
    assert not report and p.returncode == 0, p.stderr[-3000:]
    assert len(rows) == len(valid)
    wrong = [(n, r) for (n, _, d), r in zip(valid, rows) if r[0] != bc.OK or r[1] != bc.OK or r[3] != len(d)]
    assert not wrong, wrong[:10]
    p, rows = bc.core_verdicts(exe, [m for _, m in damaged], tmp_path)
    print(p.stderr[-2000:])
    report = [l for l in p.stderr.splitlines() if "Sanitizer" in l or "runtime error:" in l]
    assert not report and p.returncode == 0, p.stderr[-3000:]
    assert len(rows) == len(damaged)
    assert {r[0] for r in rows} == {bc.OK, bc.BAD_HEADER, bc.BAD_DEFLATE, bc.BAD_SIZE, bc.BAD_CRC}
    assert set(bc.FOREIGN_DAMAGED_EXPECT) == {n for n, _ in damaged}
    for (n, m), r in zip(damaged, rows):
        want = bc.FOREIGN_DAMAGED_EXPECT[n]
        if n in bc.GZIP_NOT_BGZF:  # gzip reads it, BGZF does not allow it
            assert zlib.decompress(m, 31) and want == bc.BAD_HEADER and r[0] == bc.BAD_HEADER, (n, bc.GZIP_NOT_BGZF[n], r)
        else:  # the core's status, and zlib's own verdict, are what the construction says
            assert (r[0], r[1]) == (want, want), (n, r, want)
    assert set(bc.GZIP_NOT_BGZF) <= {n for n, _ in damaged}
    # HCLEN 4 (header bits 13 .. 16 are 0) can only spell lengths of zero: no valid block has it, zlib refuses this one
    head = int.from_bytes(bc.payload_of(dict(damaged)["hclen_4"])[:3], "little")
    assert (head >> 1) & 3 == 2 and (head >> 13) & 15 == 0 and bc.FOREIGN_DAMAGED_EXPECT["hclen_4"] == bc.BAD_DEFLATE


def test_inflate_core_against_zlib_on_the_foreign_corpus(foreign, tmp_path):
    """the CPU build of the core over members that zlib's compressor never writes: OK with zlib's bytes on every valid one,
    zlib's verdict and category on every damaged one, all five statuses seen"""
    _check_foreign(bc.build_core_check(tmp_path), foreign, tmp_path)


def test_inflate_core_under_asan_and_ubsan_on_the_foreign_corpus(foreign, tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "basevar_amd", "csrc"), "../lib/san/inflate_core_check.asan"])
    _check_foreign(os.path.join(ROOT, "basevar_amd", "lib", "san", "inflate_core_check.asan"), foreign, tmp_path)


def test_new_sources_hold_no_scalar_store_mnemonics():
    """the new sources hold none of the scalar-store / scalar-cache-writeback mnemonics"""
    words = ["s_" + w for w in ("store_dword", "buffer_store_", "scratch_store_", "atomic_", "buffer_atomic_", "dcache_wb", "dcache_discard")]
    for f in ("basevar_amd/csrc/bv_inflate.hip", "basevar_amd/csrc/bv_inflate_core.h", "basevar_amd/csrc/bv_text.hip", "basevar_amd/csrc/bv_deflate.hip",
              "basevar_amd/csrc/bv_chunk_stage.h", "tests/cpp/inflate_core_check.cpp",
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
