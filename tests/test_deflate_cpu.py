"""CPU tests (no GPU) of the device DEFLATE encoder: the core the kernel compiles (basevar_amd/csrc/bv_deflate_core.h), built
with g++ under ASan + UBSan (tests/cpp/deflate_core_check.cpp), over the corpus of tests/deflate_corpus.py.  zlib, the CPU build
of the device decoder (tests/cpp/inflate_core_check.cpp) and the bit-by-bit tracer of tests/deflate_writer.py judge what it
writes; the size of what it writes is held to 2.5 times zlib's level 6 on VCF records.  Which bytes it writes is held to
tests/deflate_model.py, a serial restatement of the header's definition that shares no code with the encoder: over the edge
corpus (deflate_corpus.edge_corpus(): the window's bound, every length and distance code, the stored-or-fixed tie, the
64-position schedule, collisions, block ends) and over the corpus above, member for member, byte for byte."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzf_corpus as bc  # noqa: E402
import deflate_corpus as dc  # noqa: E402
import deflate_model as dm  # noqa: E402
import deflate_writer as dw  # noqa: E402


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """{name: (text, sizes, [members])} from the sanitized CPU build of the core"""
    d = tmp_path_factory.mktemp("deflate_core")
    emit = dc.cxx("emit_corpus", d)
    core = dc.cxx("deflate_core_check", d, sanitize=True)
    out = {}
    for name, text, sizes in dc.corpus(emit):
        raw = dc.cpu_members(core, text, sizes, d)
        members = dc.split_members(raw)
        assert len(members) == len(sizes), name
        out[name] = (text, sizes, members)
    return out


def test_every_member_inflates_to_its_block_and_states_it(coded):
    n = 0
    for name, (text, sizes, members) in coded.items():
        for m, block in zip(members, dc.blocks_of(text, sizes)):
            dc.check_member(m, block)
            n += 1
    assert n > 380
    sizes_seen = set(s for _, sizes, _ in coded.values() for s in sizes)
    assert set(range(1, 301)) <= sizes_seen and {dc.MAX_BLOCK - 1, dc.MAX_BLOCK} <= sizes_seen


def test_the_device_decoders_core_accepts_every_member(coded, tmp_path):
    exe = bc.build_core_check(tmp_path, sanitize=False)
    members = [m for _, _, ms in coded.values() for m in ms]
    p, rows = bc.core_verdicts(exe, members, tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(rows) == len(members) and all(r[0] == bc.OK and r[1] == bc.OK for r in rows)


def test_random_blocks_come_out_stored_and_text_does_not(coded):
    def stored(m):
        return (m[18] >> 1) & 3 == 0

    text, sizes, members = coded["random"]
    assert all(stored(m) and len(m) == s + 31 for m, s in zip(members, sizes))
    # (a few random bytes are shorter in the fixed code, 10 bits + 8 or 9 a byte, than behind a stored block's 5 bytes: never larger)
    text, sizes, members = coded["random_sizes_1_64"]
    assert all(len(m) <= s + 31 and (stored(m) or len(m) < s + 31) for m, s in zip(members, sizes))
    for name in ("vcf", "cvg", "rows", "one_byte"):
        assert not any(stored(m) for m in coded[name][2]), name
    # one repeated byte: a literal and matches of 258 at distance 1
    assert all(len(m) < 26 + (0xff00 // 258 + 2) * 13 // 8 + 8 for m in coded["one_byte"][2])  # 13 bits a match of 258


def test_the_tracer_finds_matches_at_short_distances_on_vcf_records(coded):
    text, sizes, members = coded["vcf"]
    tr = dw.trace(members[1][18:-8])
    assert tr.text == text[sizes[0]:sizes[0] + sizes[1]]
    assert [b[0] for b in tr.blocks] == [1]  # one block, fixed codes
    matches = [t for t in tr.tokens if not isinstance(t, int)]
    assert len(matches) > 500
    short = [t for t in matches if t[1] < 64]
    assert len(short) > 100 and any(t[1] == 4 and t[0] >= 64 for t in short)  # `\t./.` repeated
    assert any(t[1] >= 64 for t in matches)
    assert all(4 <= t[0] <= 258 and 1 <= t[1] <= 32768 for t in matches)


def test_compressed_size_of_vcf_records_against_zlib(coded):
    """The condition on the size: the members of the VCF records are at most 2.5 times what zlib's level 6 writes for the same
    blocks (a literal-only coder is at 5.8 times, zlib's level 1 with fixed codes at 1.9 times)."""
    for name in ("vcf", "cvg", "rows"):
        text, sizes, members = coded[name]
        ours = sum(len(m) for m in members)
        l6 = sum(dc.zlib_member_bytes(b, 6) for b in dc.blocks_of(text, sizes))
        l1 = sum(dc.zlib_member_bytes(b, 1) for b in dc.blocks_of(text, sizes))
        print("%s: %d bytes of text, %d in members; zlib level 6 %d (x %.3f), level 1 %d (x %.3f)" % (name, len(text), ours, l6, ours / l6, l1, ours / l1))
        if name == "vcf":
            assert ours <= 2.5 * l6


def test_the_deflate_kernel_fits_two_workgroups_on_a_cu():
    """what the kernel asks of a CU: its LDS twice inside the 160 KiB of a gfx950 CU, no scratch"""
    src = os.path.join(ROOT, "basevar_amd", "csrc", "bv_deflate.hip")
    p = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    part = p.stderr.split("bv_bgzf_deflate_kernel")[1].split("Function Name")[0]
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", part).group(1))
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", part).group(1))
    assert 0xff00 < lds <= 80 * 1024 and scratch == 0


def test_the_writers_second_way_cuts_where_the_first_does(tmp_path):
    """TextOut::write_lines with a BlockDeflater (here the CPU build of the core) against write_lines as it is, on the same
    batches of lines, under ASan + UBSan: the same inflated bytes in the same blocks, every line at the same place in its block,
    and both .tbi files point at their lines."""
    emit = dc.cxx("emit_corpus", tmp_path)
    exe = dc.cxx("deflate_writer_check", tmp_path, sanitize=True, extra=["-lz"])
    lines = tmp_path / "lines.vcf"
    lines.write_bytes(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\n" + dc.emitted(emit, "vcf", 10000, 40, 9))
    for seed in (1, 2):
        host, batch = str(tmp_path / ("host%d.vcf.gz" % seed)), str(tmp_path / ("batch%d.vcf.gz" % seed))
        p = subprocess.run([exe, str(lines), host, batch, str(seed)], capture_output=True, text=True, env=dict(os.environ, **dc.SAN_ENV), timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        calls, blocks = (int(x) for x in p.stdout.split())
        found, blocks_host, blocks_batch = dc.assert_same_text_and_places(host, batch)
        assert len(found) == 42 and calls > 3
        # every whole block but the header's went through the deflater; what it wrote is not what zlib wrote
        assert blocks == sum(1 for _, _, p in blocks_batch if len(p) == dc.MAX_BLOCK)
        assert open(host, "rb").read() != open(batch, "rb").read()


# ---------------------------------------------------------------------------------------------------------------------------
# The encoder against the model.  What these tests add, by one-line changes to bv_deflate_core.h that were each run through
# this file on the CPU build (`before`: the tests above; `model`: the two byte-for-byte tests below):
#   window `<` for `<=`                              before: all pass                      model: fails (edge corpus)
#   dist stored without `- 1`                        before: 4 of 6 fail                   model: fails
#   ... and read back without `+ 1` as well          no byte changes: 32768 fits the uint16_t, the `- 1` is a convention
#   `len == 258` case removed (284 + 31 is written)  before: the one_byte size bound fails model: fails; zlib accepts the stream
#   0x190 -> 0x191                                   before: zlib refuses the members      model: fails
#   the in-chunk candidate not taken                 before: the two size tests fail       model: fails
#   `last` always 1                                  no byte changes on one lane: the writes of step 3 run in ascending order and
#                                                    the last one stays.  On the device they are one store of 64 lanes to one
#                                                    address; there the GPU test against the model is the check
#   `measure` always true, `p >= cur` dropped        no byte changes: positions the parse has passed are measured and never read
#   the tie turned to fixed (`>` for `>=`)           before: random_sizes_1_64 fails       model: fails, edge corpus and corpus()


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    """the edge corpus: ([(name, [blocks])], every block, the sanitized CPU build's members, the model's members)"""
    d = tmp_path_factory.mktemp("deflate_edge")
    core = dc.cxx("deflate_core_check", d, sanitize=True)
    entries = dc.edge_corpus()
    text, sizes = dc.edge_text(entries)
    members = dc.split_members(dc.cpu_members(core, text, sizes, d))
    assert len(members) == len(sizes)
    blocks = list(dc.blocks_of(text, sizes))
    return entries, blocks, members, [dm.member(b) for b in blocks]


def test_the_edge_corpus_goes_where_it_is_meant_to_in_the_models_members(edge):
    """the conditions on the corpus, on what the model writes: they hold whatever the encoder does"""
    entries, blocks, _, model = edge
    for m, block in zip(model, blocks):
        dc.check_member(m, block)
    rep = dc.edge_report(model, blocks)
    dc.assert_edge_conditions(rep)
    # what single entries are for, read from the model's tokens
    at = {}
    k = 0
    for name, bs in entries:
        at[name] = [dc.traced(m) for m in model[k:k + len(bs)]]
        k += len(bs)
    window = [[t for t in tr.tokens if not isinstance(t, int) and t[1] > 30000] for tr in at["window"]]
    # (32767 and 32768 coded for both x and both tails; 32769 refused at every byte of x: literals)
    assert [[t[1] for t in w] for w in window] == [[32767]] * 3 + [[32768]] * 3 + [[]] * 3
    assert [w[0][0] for w in window[:6]] == [4, 4, 12] * 2 and at["window"][8].tokens[-14:] == list(b"klmnopqrstuv!?")
    # a shadowed repeat is literals, the same repeat without the collision a match
    coll = at["collisions"]
    n_lit = [sum(1 for t in tr.tokens if isinstance(t, int)) for tr in coll]  # (eight blocks a pair: four shadowed, four not)
    assert len(coll) % 8 == 0 and all(n_lit[k + j] > n_lit[k + 4 + j] for k in range(0, len(coll), 8) for j in range(4)), n_lit
    # the schedule's tail codes to the same tokens behind every lead (the lead's bytes are literals: they occur once)
    tails = [tr.tokens[lead:] for lead, tr in zip(list(range(64)) + [62, 63, 64, 65, 66, 126, 127, 128, 129, 130], at["schedule"])]
    assert len(tails) == 74 and all(t == tails[0] for t in tails)
    assert (258, 302) in tails[0] and (40, 158) in tails[0] and (4, 7) in tails[0] and (4, 9) in tails[0] and (4, 10) in tails[0]
    # every stored-or-fixed size of n different bytes >= 144: the first tie and the first larger one are where the bit count says
    small = at["stored_or_fixed"][:40]
    kinds = ["fixed" if tr.blocks[0][0] == 1 else "stored" for tr in small]
    first_stored = kinds.index("stored") + 1
    assert kinds == ["fixed"] * (first_stored - 1) + ["stored"] * (41 - first_stored)
    assert (10 + 9 * (first_stored - 1) + 7) // 8 < 5 + first_stored - 1 and (10 + 9 * first_stored + 7) // 8 == 5 + first_stored
    # the largest blocks: fixed at the last bit that fits, stored from the first bit of the tie
    assert ["fixed" if tr.blocks[0][0] == 1 else "stored" for tr in at["stored_or_fixed"][-6:]] == ["fixed", "stored", "stored", "stored", "fixed", "stored"]
    print("edge corpus: %d blocks, %d bytes; %d stored, %d of them ties; %d literals >= 144 beside matches; %d distances" % (
        len(blocks), sum(len(b) for b in blocks), rep["stored"], rep["ties"], rep["high_literals_beside_matches"], len(rep["distances"])))


def test_edge_members_are_the_models_byte_for_byte(edge):
    entries, blocks, members, model = edge
    names = ["%s[%d]" % (name, k) for name, bs in entries for k in range(len(bs))]
    dc.assert_members_are_the_models(names, members, model)
    dc.assert_edge_conditions(dc.edge_report(members, blocks))


def test_edge_members_inflate_with_zlib_and_with_the_device_decoders_core(edge, tmp_path):
    _, blocks, members, _ = edge
    for m, block in zip(members, blocks):
        dc.check_member(m, block)
    exe = bc.build_core_check(tmp_path, sanitize=False)
    p, rows = bc.core_verdicts(exe, members, tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(rows) == len(members) and all(r[0] == bc.OK and r[1] == bc.OK for r in rows)


def test_members_of_the_corpus_are_the_models_byte_for_byte(coded):
    """Every block of every entry of corpus(): none is left out (the model takes about a second for a megabyte of text).  For
    random_sizes_1_64 this is the exact stored-or-fixed decision where the test above asks for `stored, or smaller`."""
    n = 0
    for name, (text, sizes, members) in coded.items():
        blocks = list(dc.blocks_of(text, sizes))
        dc.assert_members_are_the_models(["%s[%d]" % (name, k) for k in range(len(blocks))], members, [dm.member(b) for b in blocks])
        n += len(blocks)
    assert n > 380
