"""CPU tests (no GPU) of the small level of the device DEFLATE encoder (BV_DEFLATE_SMALL): the core the kernel compiles
(basevar_amd/csrc/bv_deflate_small_core.h), built with g++ under ASan + UBSan as a stand-alone program
(tests/cpp/deflate_core_check.cpp --level small), over the corpus and the edge corpus of tests/deflate_corpus.py and the blocks of
tests/deflate_small_corpus.py.  Which bytes it writes is held to tests/deflate_small_model.py, a serial restatement of the
header's definition that shares no code with the encoder; zlib, the CPU build of the device decoder and the bit-by-bit tracer
of tests/deflate_writer.py read what it writes; its size is capped against zlib's level 6 and against the fast level's.

THE DEPTH LIMIT.  No text was found that drives a literal/length or distance code past 15 bits: the frequent symbols of any
text that still has matches flatten the tree (Fibonacci counts over 16 bytes would need 2,580 different 4-grams with 3.4 of
their 4 bytes from the 4 most frequent values; 256 + 3,072 such grams exist, and they average 3.1).  The limit is covered by
count vectors instead, here and on the device (bv_engine_deflate_code_lengths), against the model's lengths and rounds.

HCLEN.  The issue behind this level asks for blocks with HCLEN 4 and HCLEN 19.  Neither can be written from text: HCLEN 4 needs
a block in which no code length but 0 is spelled, and every block spells the end code's; more, a complete code over at most
30 distance symbols has a length of 4 or less, whose slot is the 12th or later: 12 is the least HCLEN of this encoder.  HCLEN
19 needs a code of exactly 15 bits, which CVG rows reach.  What is asserted: 19 over the corpus, 18 (the most without a 15-bit
code: a block without matches has the distance lengths [1, 1]) and values below it, none under 12."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzf_corpus as bc  # noqa: E402
import deflate_corpus as dc  # noqa: E402
import deflate_small_corpus as sc  # noqa: E402
import deflate_small_model as sm  # noqa: E402


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_small")
    return d, dc.cxx("emit_corpus", d), dc.cxx("deflate_core_check", d, sanitize=True)


@pytest.fixture(scope="module")
def coded(built):
    """{name: (text, sizes, [the sanitized CPU build's members], [the fast level's members])} over deflate_corpus.corpus()"""
    d, emit, core = built
    fast = dc.cxx("deflate_core_check", d)
    out = {}
    for name, text, sizes in dc.corpus(emit):
        members = dc.split_members(dc.cpu_members(core, text, sizes, d, level="small"))
        assert len(members) == len(sizes), name
        out[name] = (text, sizes, members, dc.split_members(dc.cpu_members(fast, text, sizes, d)))
    return out


@pytest.fixture(scope="module")
def edge(built):
    """both edge corpora: ([(name, [blocks])], every block, the sanitized CPU build's members, the model's members)"""
    d, emit, core = built
    entries = dc.edge_corpus() + [("small_" + name, bs) for name, bs in sc.small_edge_corpus(emit)]
    text, sizes = dc.edge_text(entries)
    members = dc.split_members(dc.cpu_members(core, text, sizes, d, level="small"))
    assert len(members) == len(sizes)
    blocks = list(dc.blocks_of(text, sizes))
    return entries, blocks, members, [sm.member(b) for b in blocks]


def test_members_of_the_corpus_are_the_models_byte_for_byte(coded):
    n = 0
    for name, (text, sizes, members, _) in coded.items():
        blocks = list(dc.blocks_of(text, sizes))
        dc.assert_members_are_the_models(["%s[%d]" % (name, k) for k in range(len(blocks))], members, [sm.member(b) for b in blocks])
        n += len(blocks)
    assert n > 380
    sizes_seen = set(s for _, sizes, _, _ in coded.values() for s in sizes)
    assert set(range(1, 301)) <= sizes_seen and {dc.MAX_BLOCK - 1, dc.MAX_BLOCK} <= sizes_seen


def test_edge_members_are_the_models_byte_for_byte(edge):
    entries, blocks, members, model = edge
    names = ["%s[%d]" % (name, k) for name, bs in entries for k in range(len(bs))]
    dc.assert_members_are_the_models(names, members, model)


def test_zlib_and_the_device_decoders_core_read_every_member_back(coded, edge, tmp_path):
    members, n = [], 0
    for name, (text, sizes, ms, _) in coded.items():
        for m, block in zip(ms, dc.blocks_of(text, sizes)):
            dc.check_member(m, block)
        members += ms
    for m, block in zip(edge[2], edge[1]):
        dc.check_member(m, block)
    members += edge[2]
    exe = bc.build_core_check(tmp_path, sanitize=False)
    p, rows = bc.core_verdicts(exe, members, tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(rows) == len(members) > 3000 and all(r[0] == bc.OK and r[1] == bc.OK for r in rows)


def test_the_tracer_reads_a_dynamic_block_with_its_declared_header(coded):
    text, sizes, members, _ = coded["vcf"]
    block = text[sizes[0]:sizes[0] + sizes[1]]
    tr = dc.traced(members[1])
    assert tr.text == block and [b[0] for b in tr.blocks] == [2]  # one block, dynamic codes
    info = {}
    assert sm.member(block, info) == members[1]
    f = tr.features
    assert f["hlit:%d" % info["hlit"]] == 1 and f["hdist:%d" % info["hdist"]] == 1 and f["hclen:%d" % info["hclen"]] == 1
    assert info["hlit"] == max(257, 1 + max(s for s in range(286) if info["ll_len"][s]))
    assert info["hdist"] == 1 + max(s for s in range(30) if info["d_len"][s])
    matches = [t for t in tr.tokens if not isinstance(t, int)]
    assert len(matches) > 300 and any(t[0] >= 16 for t in matches) and all(4 <= t[0] <= 258 and 1 <= t[1] <= 32768 for t in matches)
    assert tr.tokens == sm.tokens(block)


def test_the_new_edge_blocks_go_where_they_are_meant_to_in_the_models_members(edge):
    """the conditions on tests/deflate_small_corpus.py's blocks, on what the model writes: they hold whatever the encoder does"""
    entries, blocks, _, model = edge
    at, k = {}, 0
    for name, bs in entries:
        at[name] = (model[k:k + len(bs)], bs)
        k += len(bs)
    rep = {name[6:]: sc.small_edge_report(*at[name]) for name in at if name.startswith("small_")}
    whole = sc.small_edge_report(model, blocks)
    # every one of the three forms; the two ties: dynamic = fixed < stored is written fixed, a coded form = stored is written stored
    assert set(whole["forms"]) == {0, 1, 2} and rep["forms"]["forms"] == {2: 1, 1: 2, 0: 1}
    tie_blocks = at["small_ties"][1]
    kinds = []
    for m, b in zip(*at["small_ties"]):
        info = {}
        sm.payload(b, info)
        d, f, s = info["sizes"]
        kinds.append(("dynamic_fixed" if d == f < s else "stored" if min(d, f) == s else "none", dc.traced(m).blocks[0][0]))
    assert ("dynamic_fixed", 1) in kinds and ("stored", 0) in kinds and all(k[0] != "none" for k in kinds), (kinds, [len(b) for b in tie_blocks])
    # no match (the distance lengths [1, 1]: HDIST 2), and every match with one distance symbol
    assert rep["no_match"]["no_match_dynamic"] == 2 and rep["one_distance"]["one_distance_dynamic"] == 1
    # the header: each of 16, 17 and 18, 18 with 138; HCLEN (see the head of this file)
    f = whole["features"]
    assert f["rep18:138"] >= 1 and any(k.startswith("rep16:") for k in f) and any(k.startswith("rep17:") for k in f)
    assert {3, 6} <= {int(k.split(":")[1]) for k in f if k.startswith("rep16:")} and {3, 10} <= {int(k.split(":")[1]) for k in f if k.startswith("rep17:")}
    assert 11 in {int(k.split(":")[1]) for k in f if k.startswith("rep18:")}
    assert 18 in whole["hclen"] and min(whole["hclen"]) >= 12 and len(whole["hclen"]) >= 3, whole["hclen"]
    # a match from each table; a 16-gram candidate refused for the window and an 8-gram one for a collision, a shorter gram taken
    t = rep["tables"]
    assert t["taken"][16] >= 1 and t["taken"][8] >= 1 and t["taken"][4] >= 1
    assert t["refused"][(16, "window", 8)] >= 1 and t["refused"][(8, "collision", 4)] >= 1
    assert whole["refused"][(16, "collision", 8)] >= 1 and whole["refused"][(16, "collision", 4)] >= 1
    tokens = [dc.traced(m).tokens for m in at["small_tables"][0]]
    assert (16, 116) in tokens[0] and (11, 111) in tokens[1] and (6, 106) in tokens[2] and (8, 10) in tokens[3]
    # (the collision changes the table, not the token: the 4-gram table's candidate is the same place)
    assert (8, 136) in tokens[4] and (8, 136) in tokens[5]
    # sizes 1 .. 300 and the two largest
    assert [len(b) for b in at["small_sizes"][1]] == list(range(1, 301)) + [dc.MAX_BLOCK - 1, dc.MAX_BLOCK]
    print("small edge corpus: forms %r, HCLEN %r, taken %r, refused %r" % (dict(whole["forms"]), sorted(whole["hclen"]), dict(whole["taken"]), dict(whole["refused"])))


def test_a_header_with_hclen_19_and_a_code_of_15_bits(coded):
    text, sizes, members, _ = coded["cvg"]
    found = [dc.traced(m).features for m in members]
    assert any(f["hclen:19"] and f["hclen19_slot18_nonzero"] and (f["lit_bits:15"] or f["dist_bits:15"]) for f in found)
    assert all(4 < int(k.split(":")[1]) for f in found for k in f if k.startswith("hclen:"))


def test_a_run_of_lengths_crosses_from_the_literal_into_the_distance_lengths(edge):
    """symbol 16 repeating a literal/length code's length into the distance lengths, in the tracer's reading of the model's members"""
    _, blocks, _, model = edge
    crossing = [len(b) for m, b in zip(model, blocks) if dc.traced(m).blocks[0][0] == 2 and dc.traced(m).features["rep16_cross"]]
    assert crossing, "no member's header has a run across the two length lists"


def test_code_lengths_of_count_vectors_are_the_models(built, tmp_path):
    """the depth limit: Fibonacci counts deeper than 15 (and 7) bits, and the small cases of the construction"""
    d, _, core = built
    vectors = sc.count_vectors()
    path = tmp_path / "vectors.txt"
    path.write_text(sc.format_vectors(vectors))
    p = subprocess.run([core, "--lengths", str(path)], capture_output=True, text=True, env=dict(os.environ, **dc.SAN_ENV), timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(vectors)
    rounds_seen, named_rounds = {}, {}
    for (name, limit, counts), line in zip(vectors, lines):
        got = [int(x) for x in line.split()]
        lengths, rounds = sm.code_lengths(counts, limit)
        assert (got[1:], got[0]) == (lengths, rounds), name
        assert max(lengths) <= limit and sc.kraft_is_one(lengths), name
        assert all(l > 0 for l, c in zip(lengths, counts) if c), name
        rounds_seen.setdefault((len(counts), limit), set()).add(rounds)
        named_rounds[name] = rounds
    for key in ((286, 15), (30, 15), (19, 7)):
        assert {0, 1, 2} <= rounds_seen[key], (key, rounds_seen[key])
    # the Fibonacci vectors of one and of two rounds, by name
    assert {name: r for name, r in named_rounds.items() if name in sc.FIBONACCI_ROUNDS} == sc.FIBONACCI_ROUNDS
    named = {name: sm.code_lengths(c, limit)[0] for name, limit, c in vectors}
    assert named["no_symbol_30"] == [1, 1] + [0] * 28 and named["one_symbol_30"] == [1] + [0] * 28 + [1] and named["first_symbol_30"] == [1, 1] + [0] * 28
    assert [l for l in named["one_count_of_65281"] if l] == [1, 1] and named["one_count_of_65281"][0] == 1
    # equal counts: 285 leaves are 2^8 + 29, so the first 58 in symbol order pair up one level lower
    eq = [l for l in named["equal_286"] if l]
    assert len(eq) == 285 and eq == [9] * 58 + [8] * 227


def test_compressed_size_against_zlib_and_against_the_fast_level(coded):
    """A cap, not a measurement: VCF records, CVG rows and batchfile rows at most 1.15 times zlib's level 6 for the same blocks
    (the definition stands at 1.065 / 1.03 / 1.065), and every entry at most the fast level's size plus 4 bytes a block."""
    for name, (text, sizes, members, fast) in coded.items():
        ours, theirs = sum(len(m) for m in members), sum(len(m) for m in fast)
        l6 = sum(dc.zlib_member_bytes(b, 6) for b in dc.blocks_of(text, sizes))
        print("%s: %d bytes of text, %d in members (x %.3f of zlib level 6's %d); the fast level %d" % (name, len(text), ours, ours / l6, l6, theirs))
        if name in ("vcf", "cvg", "rows"):
            assert ours <= 1.15 * l6, name
        assert ours <= theirs + 4 * len(sizes), name
        assert all(len(m) <= s + 31 for m, s in zip(members, sizes)), name


def test_the_small_kernel_fits_a_cu_without_scratch():
    """what the kernel asks of a CU: its LDS inside the 160 KiB of a gfx950 CU -- once, where the fast level's fits twice -- and no scratch"""
    src = os.path.join(ROOT, "basevar_amd", "csrc", "bv_deflate.hip")
    p = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "bv_bgzf_deflate_kernel" not in "bv_bgzf_small_kernel"
    part = p.stderr.split("bv_bgzf_small_kernel")[1].split("Function Name")[0]
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", part).group(1))
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", part).group(1))
    print("bv_bgzf_small_kernel: %d bytes of LDS, %d workgroup(s) per CU, %d bytes of scratch a lane" % (lds, 163840 // lds, scratch))
    assert 0xff00 < lds <= 163840 and scratch == 0
