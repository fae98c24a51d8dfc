"""CPU tests (no GPU) of the rows of a region (include/basevar_amd_region.h): basevar_amd/csrc/bv_text_region_core.h -- the code
the region kernels of bv_text.hip compile -- walked in the kernels' schedule by the stand-alone harness
tests/cpp/text_region_check.cpp, built with ASan + UBSan and run as a program, against the serial model
tests/text_region_model.py on the cases of tests/text_region_corpus.py; the corpus's reach, asserted from the model's answers;
the header against the ctypes layer; and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import text_region_corpus as trc  # noqa: E402
import text_region_model as trm  # noqa: E402
from basevar_amd import _capi  # noqa: E402

CORE = os.path.join(ROOT, "basevar_amd", "csrc", "bv_text_region_core.h")
SRC = os.path.join(ROOT, "tests", "cpp", "text_region_check.cpp")
MAX_SITES = 1 << 20


def build(tmp):
    exe = os.path.join(str(tmp), "text_region_check.asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    return exe


def write_cases(path, cases):
    with open(path, "wb") as o:
        for c in cases:
            name, beg, end = c["region"]
            o.write(b"CASE %d %d %d %d %d %d\n" % (len(c["texts"]), c["at_end"], min(c["max_positions"], MAX_SITES), beg, end, len(name)) + name + b"\n")
            for t, sb, sl in zip(c["texts"], c["skip_bytes"], c["skip_lines"]):
                o.write(b"FILE %d %d %d\n" % (sb, sl, len(t)) + t + b"\n")


def answers(exe, tmp, cases, tile):
    src, dst = os.path.join(str(tmp), "cases.bin"), os.path.join(str(tmp), "answers_%d.txt" % tile)
    write_cases(src, cases)
    p = subprocess.run([exe, str(tile), src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    out = []
    for line in open(dst):
        v = [int(x) for x in line.split()]
        files = [dict(zip(("n_lines", "first", "n_in", "term", "cursor"), v[6 + 5 * f:11 + 5 * f])) for f in range((len(v) - 6) // 5)]
        out.append(dict(P=v[0], done=bool(v[1]), err=tuple(v[2:6]) if v[2] else None, files=files))
    assert len(out) == len(cases)
    return out


@pytest.fixture(scope="module")
def solved(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("text_region")
    cases = trc.cases()
    exp = [trm.select(c["texts"], c["region"], c["skip_bytes"], c["skip_lines"], c["at_end"], c["max_positions"], MAX_SITES) for c in cases]
    exe = build(tmp)
    # the kernels' tile, and tiles so small that heads cross an edge in every case (a tile of 1: every byte is one)
    return cases, exp, {tile: answers(exe, tmp, cases, tile) for tile in (16384, 1, 7, 64, 100)}


def test_core_is_the_model(solved):
    cases, exp, got = solved
    for tile, ans in got.items():
        for c, e, g in zip(cases, exp, ans):
            what = (c["name"], tile)
            assert g["err"] == e["err"], what
            assert (g["P"], g["done"]) == (e["P"], e["done"]), what
            assert [f["cursor"] for f in g["files"]] == e["cursor"], what
            if e["err"] is None:
                for gf, ef in zip(g["files"], e["files"]):
                    assert (gf["n_lines"], gf["first"], gf["n_in"], bool(gf["term"])) == (ef["n_lines"], ef["first"], ef["n_in"], ef["term"]), what


def test_corpus_reaches_its_cases(solved):
    cases, exp, _ = solved
    by = {c["name"]: (c, e) for c, e in zip(cases, exp)}
    assert len(by) == len(cases)

    def f0(name):
        return by[name][1]["files"][0]

    def pos_of(name, f=0):
        c, e = by[name]
        return [int(c["texts"][f][a:b].split(b"\t")[1]) for a, b in (r[f] for r in e["rows"])]
    for at_end in (True, False):
        e = "_end%d" % at_end
        assert (f0("ends_on_first" + e)["first"], f0("ends_on_first" + e)["n_in"], f0("ends_on_first" + e)["term"]) == (0, 1, True)
        assert (f0("ends_on_last" + e)["first"], f0("ends_on_last" + e)["n_in"], f0("ends_on_last" + e)["term"]) == (1, 1, False)
        assert (f0("ends_on_only" + e)["n_lines"], f0("ends_on_only" + e)["n_in"]) == (1, 1)
        assert by["ends_on_first" + e][1]["done"] and by["ends_on_last" + e][1]["done"] == at_end
        assert (f0("none_reached" + e)["first"], f0("none_reached" + e)["n_in"]) == (3, 0) and by["none_reached" + e][1]["cursor"] == [len(by["none_reached" + e][0]["texts"][0])]
        assert f0("all_reached" + e)["n_in"] == 3 and not f0("all_reached" + e)["term"]
        assert f0("all_skipped_other_contig" + e)["first"] == 3 and by["all_skipped_other_contig" + e][1]["done"] == at_end
        assert (f0("all_beyond" + e)["first"], f0("all_beyond" + e)["n_in"], by["all_beyond" + e][1]["done"]) == (0, 0, True)
        assert by["empty_file" + e][1]["P"] == 0 and by["empty_file" + e][1]["files"][0]["n_lines"] == 0
        assert by["empty_file" + e][1]["err"] == ((trm.ERR_COUNT, 0, 0, 1) if at_end else None)  # (at its end, an empty file has terminated)
        assert by["nothing_behind_skip" + e][1]["cursor"][0] == by["nothing_behind_skip" + e][0]["skip_bytes"][0]
    assert pos_of("beg_and_end_edges") == [10, 11, 19, 20]
    assert by["beg_minus_1_only"][1]["P"] == 0 and f0("beg_minus_1_only")["first"] == 1
    assert by["end_plus_1_only"][1]["P"] == 0 and (f0("end_plus_1_only")["first"], f0("end_plus_1_only")["term"]) == (0, True)
    assert (f0("name_prefix_and_extension")["first"], f0("name_prefix_and_extension")["n_in"], f0("name_prefix_and_extension")["term"]) == (2, 1, True)
    assert f0("name_is_prefix_only")["first"] == 3 and by["name_is_prefix_only"][1]["P"] == 0
    c, e = by["contig_before_and_behind"]
    assert [f["first"] for f in e["files"]] == [3, 1] and e["P"] == 3 and e["done"] and all(f["term"] for f in e["files"])
    assert f0("contig_behind_only")["first"] == 1 and pos_of("contig_behind_only") == [2, 3]
    assert pos_of("pos_1_9_10_digits") == [5, 123456789, 1234567890, 4294967295]
    assert pos_of("pos_10_digits_zero_padded") == [15]
    for label, bad in trc.MALFORMED:
        assert trm.head(bad) is None
        assert by["mal_front_" + label][1]["err"] == (trm.ERR_HEAD, 0, 1, 0)
        assert by["mal_inside_" + label][1]["err"] == (trm.ERR_HEAD, 0, 2, 0)
        assert by["mal_ending_" + label][1]["err"] == (trm.ERR_HEAD, 0, 3, 0)
        assert by["mal_behind_" + label][1]["err"] is None and by["mal_behind_" + label][1]["P"] == 3 and by["mal_behind_" + label][1]["done"]
        assert by["mal_second_file_" + label][1]["err"] == (trm.ERR_HEAD, 1, 3, 0)
        assert by["mal_nothing_reached_" + label][1]["err"] == (trm.ERR_HEAD, 0, 1, 0)
    assert [by["max_positions_%d_n_in_7" % mp][1]["P"] for mp in (1, 6, 7, 8, 100)] == [1, 6, 7, 7, 7]
    assert [by["max_positions_%d_n_in_7" % mp][1]["done"] for mp in (1, 6, 7, 8, 100)] == [False, False, True, True, True]
    assert by["count_disagrees"][1]["err"] == (trm.ERR_COUNT, 1, 5, 0)
    assert by["count_disagrees_at_end"][1]["err"] == (trm.ERR_COUNT, 1, 5, 0)
    assert by["count_open_not_at_end"][1]["err"] is None and by["count_open_not_at_end"][1]["P"] == 5 and not by["count_open_not_at_end"][1]["done"]
    assert by["count_disagrees_at_cap"][1]["err"] is None and by["count_disagrees_at_cap"][1]["P"] == 5
    assert by["count_disagrees_below_cap"][1]["err"] == (trm.ERR_COUNT, 1, 5, 0)
    assert by["one_file_has_nothing"][1]["err"] == (trm.ERR_COUNT, 1, 0, 0)
    assert by["pos_disagrees"][1]["err"] == (trm.ERR_POS, 1, 3, 0)
    assert by["pos_disagrees_third_file"][1]["err"] == (trm.ERR_POS, 2, 6, 0)
    assert by["pos_disagrees_behind_cap"][1]["err"] is None and by["pos_disagrees_behind_cap"][1]["P"] == 3
    assert by["header_lines"][1]["P"] == 7 and by["header_bytes_and_lines"][1]["P"] == 7
    c, e = by["fewer_lines_than_header_lines"]
    assert e["files"][0]["n_lines"] == 0 and e["cursor"][0] == 0 and e["P"] == 0 and not e["done"]
    assert by["only_header_lines"][1]["files"][0]["n_lines"] == 0 and by["only_header_lines"][1]["err"] == (trm.ERR_COUNT, 0, 0, 1)
    assert [by["no_last_newline_inside_end%d" % a][1]["P"] for a in (1, 0)] == [4, 3]
    assert [by["no_last_newline_terminating_end%d" % a][1]["done"] for a in (1, 0)] == [True, False]
    assert [by["no_last_newline_only_line_end%d" % a][1]["files"][0]["n_lines"] for a in (1, 0)] == [1, 0]
    c, e = by["long_middle"]
    assert len(c["texts"][0]) > 3 * 16384 and e["P"] == 801 and [f["first"] for f in e["files"]] == [1200, 505] and e["done"]
    assert e["rows"][0][0][0] // 16384 == 1 and e["rows"][-1][0][0] // 16384 == 2  # a tile of skipped lines in front, rows in two tiles
    assert by["long_chained_cap"][1]["P"] == 900 and not by["long_chained_cap"][1]["done"]
    assert by["long_to_the_end"][1]["P"] == 10 and not by["long_to_the_end"][1]["done"]
    assert pos_of("long_chrom") == [5] and by["long_line_without_tab_behind"][1]["P"] == 1
    # the seeded cases: every outcome; the long cases: rows that begin at every byte of a 64-byte step
    rnd = [(c, e) for c, e in zip(cases, exp) if c["name"].startswith("random_")]
    assert {e["err"][0] if e["err"] else 0 for c, e in rnd} == {0, trm.ERR_HEAD, trm.ERR_COUNT, trm.ERR_POS}
    assert sum(e["P"] > 0 for c, e in rnd) > 60 and sum(e["done"] for c, e in rnd) > 60 and sum(not e["done"] and e["err"] is None for c, e in rnd) > 30
    for name in ("long_",):
        some = [(c, e) for c, e in zip(cases, exp) if c["name"].startswith(name)]
        assert {(r[f][0] - c["skip_bytes"][f]) % 64 for c, e in some for r in e["rows"] for f in range(len(r))} == set(range(64)), name


def test_header_matches_ctypes():
    text = open(os.path.join(ROOT, "include", "basevar_amd_region.h")).read()
    declared = sorted(set(re.findall(r"^int (bv_\w+)\(", text, re.M)))
    assert declared == sorted(_capi.REGION_EXPORTS) == ["bv_engine_text_parse_bgzf_region"]
    lib = _capi.load()
    assert hasattr(lib, declared[0])
    body = re.search(r"typedef struct bv_text_region \{(.*?)\} bv_text_region;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == [f for f, _ in _capi.TextRegion._fields_]
    assert C.sizeof(_capi.TextRegion) == 24
    assert '#include "basevar_amd_bgzf.h"' in text


def test_region_kernels_use_no_scratch():
    """The compiler's resource summary of bv_text.hip: the three region kernels have a private segment of 0 and no spilled
    register; the head kernel holds no LDS; the one atomic is the POS check's 32-bit atomicMin"""
    src = os.path.join(ROOT, "basevar_amd", "csrc", "bv_text.hip")
    p = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    chunks = out.split("Function Name: ")[1:]  # one per kernel: its name, then its figures
    region = {c.split()[0]: c for c in chunks if "bv_text_region_" in c.split()[0]}
    assert len(region) == 3 and all(sum(w in k for k in region) == 1 for w in ("head", "combine", "pos"))
    for k, v in region.items():
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", v).group(1)) == 0, k
        assert int(re.search(r"VGPRs Spill: (\d+)", v).group(1)) == 0 and int(re.search(r"SGPRs Spill: (\d+)", v).group(1)) == 0, k
        assert int(re.search(r" VGPRs: (\d+)", v).group(1)) <= 64, k
        if "head" in k or "pos" in k:
            assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", v).group(1)) == 0, k
    core = open(CORE).read()
    assert "atomic" not in core and "printf" not in core
    kernels = re.search(r"__global__[^\n]*bv_text_region_head_kernel.*?// ---- bv_engine_text_rows_fetch", open(src).read(), re.S).group(0)
    assert kernels.count("atomic") == 1 and "atomicMin(err, r)" in kernels
