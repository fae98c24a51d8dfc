"""The text that the device DEFLATE encoder (basevar_amd/csrc/bv_deflate_core.h) is held to, on the CPU (tests/test_deflate_cpu.py)
and on the GPU (tests/test_gpu_bgzf_deflate.py), and the CPU build of the encoder that both compare against: VCF records and
CVG rows as host/vcf_emit.hpp writes them (tests/cpp/emit_corpus.cpp), batchfile rows, one repeated byte, random bytes, every
block size from 1 to 300 and the two largest."""
import os
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BLOCK = 0xff00
EOF_MARKER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
SAN_FLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SAN_ENV = dict(ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")


def cxx(name, out_dir, sanitize=False, extra=()):
    """tests/cpp/<name>.cpp compiled with g++ (plain, or ASan + UBSan)"""
    exe = os.path.join(str(out_dir), name + (".asan" if sanitize else ""))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include")] + (SAN_FLAGS if sanitize else ["-O2"]) +
                          [os.path.join(ROOT, "tests", "cpp", name + ".cpp")] + list(extra) + ["-o", exe])
    return exe


def emitted(exe, kind, samples, lines, seed):
    """`lines` VCF records or CVG rows of `samples` samples, as host/vcf_emit.hpp writes them"""
    return subprocess.check_output([exe, kind, str(samples), str(lines), str(seed)])


def whole_blocks(n, block=MAX_BLOCK):
    return [min(block, n - at) for at in range(0, n, block)]


def corpus(emit_exe):
    """[(name, text, [block sizes])]; the sizes of an entry add up to its text"""
    import bgzf_corpus as bc
    rng = np.random.default_rng(17)
    vcf = emitted(emit_exe, "vcf", 10000, 10, 5)      # ten records of about 50 KB: what a 10,000-sample call writes
    cvg = emitted(emit_exe, "cvg", 10000, 3000, 6)
    rows = bc.rows_text(150000, seed=8)
    small = emitted(emit_exe, "vcf", 1000, 12, 7)
    assert len(small) >= 45150 and len(vcf) > 6 * MAX_BLOCK
    out = [("vcf", vcf, whole_blocks(len(vcf))), ("cvg", cvg, whole_blocks(len(cvg))), ("rows", rows, whole_blocks(len(rows))),
           ("one_byte", b"a" * (MAX_BLOCK + 777), whole_blocks(MAX_BLOCK + 777)),
           ("random", rng.integers(0, 256, 2 * MAX_BLOCK + 999, dtype=np.uint8).tobytes(), [MAX_BLOCK, MAX_BLOCK - 1, 1000]),
           ("sizes_1_300", small[:45150], list(range(1, 301))),
           ("random_sizes_1_64", rng.integers(0, 256, 2080, dtype=np.uint8).tobytes(), list(range(1, 65))),
           ("largest", vcf[:2 * MAX_BLOCK - 1], [MAX_BLOCK - 1, MAX_BLOCK]),
           ("odd_cut", vcf[3:3 + 100001], whole_blocks(100001, 33333))]
    for name, text, sizes in out:
        assert sum(sizes) == len(text) and all(1 <= s <= MAX_BLOCK for s in sizes), name
    return out


def cpu_members(core_exe, text, sizes, work_dir, sanitize_env=True):
    """the CPU build of the core over the blocks: the members, back to back"""
    tp, op, sp = (os.path.join(str(work_dir), n) for n in ("text.bin", "members.bin", "sizes.txt"))
    with open(tp, "wb") as fh:
        fh.write(text)
    with open(sp, "w") as fh:
        fh.write("\n".join(str(s) for s in sizes) + "\n")
    p = subprocess.run([core_exe, tp, op, "@" + sp], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV), timeout=1200)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    with open(op, "rb") as fh:
        return fh.read()


def split_members(raw):
    """the members of a run, cut by their BSIZE fields"""
    out, at = [], 0
    while at < len(raw):
        assert raw[at:at + 16] == EOF_MARKER[:16], "not a BGZF header at %d" % at
        size = struct.unpack_from("<H", raw, at + 16)[0] + 1
        assert at + size <= len(raw)
        out.append(raw[at:at + size])
        at += size
    return out


def check_member(m, block):
    """one member against its text: zlib inflates the payload to the text and ends exactly at its end; CRC32, ISIZE, BSIZE, size"""
    assert 26 <= len(m) <= 65536 and len(m) <= len(block) + 31
    assert struct.unpack_from("<H", m, 16)[0] + 1 == len(m)
    d = zlib.decompressobj(-15)
    text = d.decompress(m[18:-8])
    assert text == block and d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    assert struct.unpack("<II", m[-8:]) == (zlib.crc32(block) & 0xFFFFFFFF, len(block))


def blocks_of(text, sizes):
    at = 0
    for s in sizes:
        yield text[at:at + s]
        at += s


def zlib_member_bytes(block, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return 18 + len(co.compress(block) + co.flush()) + 8


def indexed_lines(gz):
    """the lines of a BGZF file as tests/bam_py.py finds them by a linear scan, [(virtual offset, virtual offset behind, line)],
    after checking that the .tbi beside the file points at every data line: its leaf bin has a chunk that covers the line's
    offsets, the linear index of its 16 kb window does not start behind it, the chunks tile the data lines in file order and
    the pseudo-bin counts them (what tests/test_host_formats.py asks of the host writer's index)"""
    import bam_py
    lines = bam_py.bgzf_lines(gz)
    recs = [(s, e, l.split(b"\t", 2)) for s, e, l in lines if not l.startswith(b"#")]
    tbi = bam_py.read_tbi(gz + ".tbi")
    by_ref = {}
    for s, e, c in recs:
        by_ref.setdefault(c[0].decode(), []).append((int(c[1]), s, e))
    assert tbi["conf"] == (1, 1, 2, 0, ord("#"), 0) and tbi["names"] == list(by_ref)
    for name, ref in zip(tbi["names"], tbi["refs"]):
        mine = by_ref[name]
        bins = dict(ref["bins"])
        meta = bins.pop(37450)
        assert meta[0] == (mine[0][1], mine[-1][2]) and meta[1] == (len(mine), 0)
        chunks = sorted(c for cs in bins.values() for c in cs)
        assert all(a[1] <= b[0] for a, b in zip(chunks, chunks[1:]))
        assert chunks[0][0] == mine[0][1] and chunks[-1][1] == mine[-1][2]
        for pos, s, e in mine:
            beg = pos - 1
            assert any(cb <= s and e <= ce for cb, ce in bins.get(4681 + (beg >> 14), [])), (name, pos)
            assert ref["linear"][beg >> 14] <= s
    return lines


def assert_same_text_and_places(host_gz, other_gz):
    """two BGZF files of the same lines, cut at the same places: the same inflated bytes, the same number of members, every
    line at the same offset inside its block (the low 16 bits of its virtual offsets), both indexes pointing at their lines"""
    import bam_py
    a, b = indexed_lines(host_gz), indexed_lines(other_gz)
    assert [l for _, _, l in a] == [l for _, _, l in b]
    assert [(s & 0xffff, e & 0xffff) for s, e, _ in a] == [(s & 0xffff, e & 0xffff) for s, e, _ in b]
    ba, bb = bam_py.bgzf_blocks(host_gz), bam_py.bgzf_blocks(other_gz)
    assert [p for _, _, p in ba] == [p for _, _, p in bb]
    # the blocks before a line are the same in number: the high bits name the same block
    index_a = {off: k for k, (off, _, _) in enumerate(ba)}
    index_b = {off: k for k, (off, _, _) in enumerate(bb)}
    assert [index_a[s >> 16] for s, _, _ in a] == [index_b[s >> 16] for s, _, _ in b]
    return a, ba, bb
