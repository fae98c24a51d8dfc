"""CPU tests (no GPU) of the device DEFLATE encoder: the core the kernel compiles (basevar_amd/csrc/bv_deflate_core.h), built
with g++ under ASan + UBSan (tests/cpp/deflate_core_check.cpp), over the corpus of tests/deflate_corpus.py.  zlib, the CPU build
of the device decoder (tests/cpp/inflate_core_check.cpp) and the bit-by-bit tracer of tests/deflate_writer.py judge what it
writes; the size of what it writes is held to 2.5 times zlib's level 6 on VCF records."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzf_corpus as bc  # noqa: E402
import deflate_corpus as dc  # noqa: E402
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
