"""CPU tests (no GPU) of the device's text tokens (include/basevar_amd_text_tokens.h): basevar_amd/csrc/bv_text_tokens_core.h --
the code the kernels of bv_text_tokens.hip compile -- against the host reader and BaseTypeEngine::finish_text's walk inside the
stand-alone harness tests/cpp/text_tokens_check.cpp, built with ASan + UBSan and run as a program; a serial model against the
harness's dump; the corpus's reach, asserted from that dump and the rows' bytes; the header against the ctypes layer; and the
kernels' resources."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import text_tokens_model as ttm  # noqa: E402
from basevar_amd import _capi  # noqa: E402


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    batches = ttm.corpus()
    return batches, ttm.run(ttm.build(asan=True), batches, tmp_path_factory.mktemp("text_tokens"))


def test_core_is_the_host_readers_and_the_model(dumped):
    """(the harness has exited non-zero if the core parts from parse_site_rows_fast or from finish_text's walk on any position)"""
    batches, dump = dumped
    for b, got in zip(batches, dump):
        assert [(p, s, t) for p, s, f, t in got] == b.tokens(), b.name
        assert [p for p, s, f, t in got] == sorted(p for p, s, f, t in got)


def test_corpus_reaches_its_cases(dumped):
    batches, dump = dumped
    by = {b.name: (b, d) for b, d in zip(batches, dump)}
    # files, samples, positions
    assert {b.F for b in batches} >= {1, 2, 3}
    assert {n for b in batches for n in b.file_samples} >= {1, 2, 63, 64, 65, 200}
    assert {b.P for b in batches} >= {1, 2, 65}
    # where the dumped tokens stand in their rows: first byte and ending separator, by lane of the 64-byte steps from the row's start
    places = []
    for b, d in zip(batches, dump):
        seen = {}
        for p, s, f, t in d:
            k = seen.get((p, f), 0)
            seen[(p, f)] = k + 1
            beg, end = ttm.token_places(b.rows[p][f])[k]
            assert b.rows[p][f][beg:end] == t
            places.append((beg, end))
    assert {beg % 64 for beg, end in places} == set(range(64))
    assert {end % 64 for beg, end in places} == set(range(64))
    assert any(beg % 64 == 63 and end > beg + 1 for beg, end in places)              # begins on lane 63 and goes on in the next step
    assert any(end % 64 == 0 and beg // 64 == end // 64 - 1 for beg, end in places)  # ended by lane 0 of the next step
    assert any(end // 64 - beg // 64 >= 100 for beg, end in places)                  # spans a hundred steps and more
    # lengths
    lens = {len(t) for d in dump for p, s, f, t in d}
    assert lens >= {1, 2, 63, 64, 65, 129, 9000}
    assert {t for d in dump for p, s, f, t in d} >= {b"+", b"-"}
    b, d = by["lengths"]
    assert any(a[0] == c[0] and a[1] + 1 == c[1] and len(a[3]) == len(c[3]) == 9000 for a, c in zip(d, d[1:]))  # back to back
    # places in the column: the first, the last (ended by the tab), the only token; every sample; alternating
    foff = [0, 63, 128]
    assert (1, foff[0], 0, b"-TT") in d and (1, foff[0] + 62, 0, b"+GGG") in d and b.rows[1][0].split(b"\t")[5].endswith(b" +GGG")
    assert [s for p, s, f, t in d if (p, f) == (0, 1)] == list(range(63, 128))
    col = b.rows[0][2].split(b"\t")[5].split(b" ")
    assert col[:4] == [b"+A", b"N", b"-C", b"N"] and [s - 128 for p, s, f, t in d if (p, f) == (0, 2)] == list(range(0, 200, 2))
    assert not any((p, f) == (1, 2) for p, s, f, t in d) and not ttm.marked(b.rows[1][2])
    assert by["only"][1] == [(0, 0, 0, b"+ACG")]
    # what must not be taken: the bytes are there, the tokens are not
    b, d = by["not_taken"]
    assert d == [(0, 2, 0, b"+T")]
    for files in b.rows:
        for row in files:
            f = row.split(b"\t")
            assert b"-" in f[0] and b"+" in f[0] and f[2] in (b"+", b"-")
            assert set(f[8].split(b" ")) <= {b"+", b"-"} and {b"+", b"-"} & set(f[6].split(b" "))
            assert all(t.isdigit() for t in f[4].split(b" ") + f[7].split(b" "))
    b, d = by["none"]
    assert d == [] and all(b"+" in row.split(b"\t")[6] and b"-" in row.split(b"\t")[8] for files in b.rows for row in files)
    # states: each kind with marked rows of kept positions before and after
    b, d = by["states"]
    kept = {p for p, s, f, t in d}
    assert kept == {p for p in range(b.P) if b.state[p] == 0}
    odd = [p for p in range(b.P) if b.state[p]]
    assert [b.state[p] for p in odd] == [ttm.SKIP, ttm.HOST, ttm.HOST, ttm.HOST, ttm.SKIP] and b.host_skips == {9}
    for p in odd:
        assert p - 1 in kept and p + 1 in kept and any(ttm.marked(r) for r in b.rows[p]), p
    assert sum(int(r.split(b"\t")[3]) for r in b.rows[1]) == 0                               # Depth sums to 0
    assert ttm.marked(b.rows[3][0]) and b"AC" in b.rows[3][2].split(b"\t")[5].split(b" ")   # file 2's defect behind file 0's marked row
    assert b"." in [s for s, c in zip(b.rows[5][1].split(b"\t")[8].split(b" "), b.rows[5][1].split(b"\t")[5].split(b" ")) if c in (b"A", b"C", b"G", b"T")]
    assert b.rows[7][0].index(b"\t", b.rows[7][0].index(b"\t", b.rows[7][0].index(b"\t") + 1) + 1) > 512  # the prefix
    assert [int(files[0].split(b"\t")[1]) for files in b.rows] == sorted((int(files[0].split(b"\t")[1]) for files in b.rows), reverse=True)  # POS descends
    # chunks: the parse's own cut (whole positions, bv_engine_text_parse) gives 3 chunks and more, marked rows first and last
    b, d = by["chunks"]
    # (on an engine whose stage is no larger yet: the GPU tests run this batch on an engine of its own and assert the same cut)
    chunks = b.chunks()
    assert len(chunks) >= 3 and all(ttm.marked(b.rows[p0][0]) and ttm.marked(b.rows[p1 - 1][-1]) for p0, p1 in chunks)
    assert len(b.chunks(cap_before=1 << 14)) == 1  # ... and why: a stage that has grown takes the batch whole
    for p0, p1 in chunks[1:]:  # a token that spans steps in every later chunk
        assert any(len(t) > 64 for p, s, f, t in d if p0 <= p < p1)
    assert {p for p, s, f, t in d} == set(range(b.P))
    # the reference's own rows
    assert sum(len(d) for b, d in zip(batches, dump) if b.name.startswith("golden_")) > 100
    assert any(ttm.SKIP in b.state for b in batches if b.name.startswith("golden_"))


def test_header_matches_ctypes():
    """include/basevar_amd_text_tokens.h: its exports are the library's and the ctypes layer's"""
    text = open(os.path.join(ROOT, "include", "basevar_amd_text_tokens.h")).read()
    declared = sorted(set(re.findall(r"^int (bv_\w+)\(", text, re.M)))
    assert declared == sorted(_capi.TEXT_TOKENS_EXPORTS) and len(declared) == 4
    others = (set(_capi.EXPORTS) | set(_capi.BGZF_EXPORTS) | set(_capi.VCF_EXPORTS) | set(_capi.RECORD_TEXT_EXPORTS) | set(_capi.INDEL_EXPORTS) |
              set(_capi.PILEUP_EXPORTS) | set(_capi.PILEUP_TEXT_EXPORTS) | set(_capi.PILEUP_BGZF_EXPORTS))
    assert not set(declared) & others
    lib = _capi.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert '#include "basevar_amd_indel.h"' in text
    core = open(ttm.CORE).read()
    body = re.search(r"struct bv_tt_token \{(.*?)\};", core, re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", body) == [f for f in _capi.PILEUP_TOKEN_DTYPE.names]
    assert C.sizeof(_capi.IndelTokens) == 40


def test_kernels_use_no_scratch():
    """The compiler's resource summary of bv_text_tokens.hip: a private segment of 0 and no spilled register in any kernel, no
    LDS in the walk, no atomics anywhere"""
    src = os.path.join(ROOT, "basevar_amd", "csrc", "bv_text_tokens.hip")
    p = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    kernels = re.findall(r"Function Name: (\S+)", out)
    assert len(kernels) == 4 and all(sum(w in k for k in kernels) == 1 for w in ("count", "write", "scan", "pack"))
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)] == [0] * 4
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out)] == [0] * 4 and [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", out)] == [0] * 4
    assert max(int(x) for x in re.findall(r" VGPRs: (\d+)", out)) <= 64
    lds = dict(zip(kernels, (int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out))))
    assert all(v == 0 for k, v in lds.items() if "scan" not in k)
    text = open(src).read() + open(ttm.CORE).read()
    assert "atomic" not in text.replace("No atomics", "") and "printf" not in text
