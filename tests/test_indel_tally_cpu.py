"""CPU tests (no GPU) of the device's indel tally (include/basevar_amd_indel.h): basevar_amd/csrc/bv_indel_tally_core.h -- the
code the kernels of bv_indel_tally.hip compile -- against host/vcf_emit.hpp's indel_string inside the stand-alone harness
tests/cpp/indel_tally_check.cpp, built with ASan + UBSan and run as a program; a serial model against the harness's dump; the
corpus's reach, asserted from that dump; the header against the ctypes layer; and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import indel_tally_ref as ref  # noqa: E402
import record_text_model  # noqa: E402
from basevar_amd import _capi  # noqa: E402


@pytest.fixture(scope="module")
def exe():
    return ref.build(asan=True)


@pytest.fixture(scope="module")
def dumped(exe, tmp_path_factory):
    rows = ref.corpus()
    return rows, ref.run_rows(exe, rows, tmp_path_factory.mktemp("indel_tally"))


def test_order_is_std_strings(exe):
    """bv_it_cmp, keys and bytes, on pairs that differ at every place around the key's edge and at the text's end, by every edge
    byte value, on proper prefixes, and on texts of 9,000 bytes"""
    assert ref.run_order(exe) > 10 ** 6


def test_core_is_indel_string_and_the_model(dumped):
    """(the harness has exited non-zero if the core and indel_string part on any row)"""
    rows, dump = dumped
    want = rows.expected()
    assert len(dump) == len(rows.keys) == len(want)
    for k, ((flag, n, classes, most, column), (mflag, mcolumn)) in enumerate(zip(dump, want)):
        assert (flag, column) == (mflag, mcolumn), (k, int(rows.keys[k]))
        assert n == len(rows.tokens_of(rows.keys[k]))
        if not flag:
            assert record_text_model.indel_column(rows.tokens_of(rows.keys[k])) == (column or b".")


def test_corpus_reaches_its_cases(dumped):
    rows, dump = dumped
    by_pos = {int(k): d for k, d in zip(rows.keys, dump)}
    row = lambda name: by_pos[rows.names[name]]  # noqa: E731
    col = lambda name: row(name)[4]  # noqa: E731
    # order
    assert col("plus_minus") == b"+AT|1,-AT|2"
    assert col("prefix") == b"+A|2,+AC|1,+ACG|1"
    assert col("high_byte_in_key") == b"+Aa|1,+A\x7f|1,+A\x80|1,+A\xff|1"  # (a signed compare puts 0x80 and 0xff first)
    assert col("high_byte_beyond_key").split(b",")[0] == b"+ACGT|1" and col("high_byte_beyond_key").index(b"+ACGTaT") < col("high_byte_beyond_key").index(b"+ACGT\x80T")
    for k in (15, 16, 17, 63, 64, 65):
        entries = col("equal_to_%d" % k).split(b",")
        assert [len(e) for e in entries] == [k - 1 + 2, k + 2, k + 2] and entries[1].endswith(b"g|2") and entries[2].endswith(b"t|1")
    assert col("one_byte") == b"+|2,+A|1,-|1"
    assert col("long_equal").endswith(b"|2") and len(col("long_equal")) == 9002
    assert row("long_last_byte")[:3] == (1, 2, 2)
    # row sizes, and the limit
    for n in (1, 2, 63, 64, 65, 127, 128, 129, ref.LIMIT - 1, ref.LIMIT):
        assert row("size_%d" % n)[:2] == (0, n) and col("size_%d" % n)
    assert row("size_%d" % (ref.LIMIT + 1))[:2] == (1, ref.LIMIT + 1) and not col("size_%d" % (ref.LIMIT + 1))
    assert ref.LIMIT >= 4096 and ref.LIMIT == _capi.load().bv_indel_row_tokens_max()
    # classes
    for c in (1, 2, 63, 64, 65):
        assert row("classes_%d" % c)[:3] == (0, 2 * c + 1, c)
    for n in (64, 65, 300):
        assert row("all_distinct_%d" % n)[:4] == (0, n, n, 1)
    # counts
    assert sorted(int(e.rsplit(b"|", 1)[1]) for e in col("counts").split(b",")) == [1, 9, 10, 99, 100, 9999]
    assert col("count_10000") == b"-G|10000"
    # column lengths
    assert (row("column_16384_one")[0], len(col("column_16384_one"))) == (0, 16384) and row("column_16385_one")[0] == 1
    assert (row("column_16384_many")[0], len(col("column_16384_many")), row("column_16384_many")[2]) == (0, 16384, 3277)
    assert row("column_16385_many")[0] == 1 and row("column_16385_many")[2:4] == (3277, 10)
    assert len(ref.model_column(rows.tokens_of(rows.names["column_16385_many"]))) == 16385 == len(ref.model_column(rows.tokens_of(rows.names["column_16385_one"])))
    # the filter
    assert col("filter") == b"+A|2,-C|1" and row("filter")[:3] == (0, 11, 2) and row("filter_all") == (0, 3, 0, 0, b"")
    # alignment: kept tokens of asked rows begin at every offset modulo 16
    asked = set(int(k) for k in rows.keys)
    assert {int(t["text_off"]) % 16 for t in rows.tokens if int(t["pos"]) in asked and int(t["text_len"])} == set(range(16))
    # keys
    keys = [int(k) for k in rows.keys]
    assert col("shuffle_a") == col("shuffle_b") and rows.tokens_of(rows.names["shuffle_a"]) != rows.tokens_of(rows.names["shuffle_b"])
    assert rows.names["unasked"] not in asked and (rows.tokens["pos"] == rows.names["unasked"]).sum() == 7
    empty = [i for i, k in enumerate(keys) if not rows.tokens_of(k)]
    assert any(0 < i < len(keys) - 1 and rows.tokens_of(keys[i - 1]) and rows.tokens_of(keys[i + 1]) for i in empty)
    assert {5, 0xffffffff} <= set(keys) and int(rows.tokens["pos"].max()) < 0xffffffff
    assert keys.count(rows.names["plus_minus"]) >= 3 and any(a > b for a, b in zip(keys, keys[1:])) and any(a < b for a, b in zip(keys, keys[1:]))
    # seeded rows over the whole byte range
    seen = set()
    for name, p in rows.names.items():
        if name.startswith("seeded_"):
            seen |= set(b"".join(rows.tokens_of(p)))
            assert by_pos[p][0] == 0
    assert len(seen) == 256


def test_header_matches_ctypes():
    """include/basevar_amd_indel.h: its exports are the library's, its struct is _capi's"""
    text = open(os.path.join(ROOT, "include", "basevar_amd_indel.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|uint32_t) (bv_\w+)\(", text, re.M)))
    assert declared == sorted(_capi.INDEL_EXPORTS) and len(declared) == 4
    others = set(_capi.EXPORTS) | set(_capi.BGZF_EXPORTS) | set(_capi.VCF_EXPORTS) | set(_capi.RECORD_TEXT_EXPORTS) | set(_capi.PILEUP_EXPORTS) | set(_capi.PILEUP_TEXT_EXPORTS)
    assert not set(declared) & others
    lib = _capi.load()
    for name in declared:
        assert hasattr(lib, name), name
    body = re.search(r"typedef struct bv_indel_tokens \{(.*?)\} bv_indel_tokens;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*?(\w+)\s*[,;]", body) == [f for f, _ in _capi.IndelTokens._fields_]
    assert C.sizeof(_capi.IndelTokens) == 2 * 8 + 2 * 8 + 2 * 4
    assert ref.TOKEN_DTYPE == _capi.PILEUP_TOKEN_DTYPE
    core = open(ref.CORE).read()
    assert int(re.search(r"#define BV_IT_COLUMN_MAX (\d+)u", core).group(1)) == _capi.RECORD_TEXT_INDEL_MAX == ref.COLUMN_MAX


def test_kernels_use_no_scratch():
    """The compiler's resource summary of bv_indel_tally.hip: a private segment of 0 and no spilled register in any kernel"""
    src = os.path.join(ROOT, "basevar_amd", "csrc", "bv_indel_tally.hip")
    p = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    kernels = re.findall(r"Function Name: (\S+)", out)
    assert len(kernels) == 3 and sum("count" in k for k in kernels) == 1 and sum("write" in k for k in kernels) == 1 and sum("check" in k for k in kernels) == 1
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)] == [0, 0, 0]
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out)] == [0, 0, 0] and [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", out)] == [0, 0, 0]
    assert max(int(x) for x in re.findall(r" VGPRs: (\d+)", out)) <= 128
    text = open(src).read() + open(ref.CORE).read()
    assert "atomic" not in text.replace("No atomics", "") and "printf" not in text
