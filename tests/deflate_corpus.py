"""The text that the device DEFLATE encoder (basevar_amd/csrc/bv_deflate_core.h) is held to, on the CPU (tests/test_deflate_cpu.py)
and on the GPU (tests/test_gpu_bgzf_deflate.py), and the CPU build of the encoder that both compare against: VCF records and
CVG rows as host/vcf_emit.hpp writes them (tests/cpp/emit_corpus.cpp), batchfile rows, one repeated byte, random bytes, every
block size from 1 to 300 and the two largest (corpus()); and an edge corpus of blocks built for the encoder's bounds (edge_corpus()),
whose expected members come from tests/deflate_model.py."""
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


# ---------------------------------------------------------------------------------------------------------------------------
# The edge corpus: blocks built for the places where an LZ77 coder goes wrong and the text above does not go -- the window's
# bound, every match length and distance code, 9-bit literals beside matches, the stored-or-fixed decision at its tie, the
# encoder's 64-position schedule, hash collisions, block ends.  tests/deflate_model.py says what every block becomes;
# edge_report() says, from the tracer's reading of the members, whether the corpus went where it was meant to go.

LETTERS = b"wxyz"


def _rand(rng, k, lo=0, hi=256):
    return rng.integers(lo, hi, k, dtype=np.uint8).tobytes()


def _distinct(rng, k, lo, hi):
    """k different bytes of lo .. hi - 1, shuffled: no four of them occur twice"""
    assert k <= hi - lo
    return rng.permutation(np.arange(lo, hi, dtype=np.uint8))[:k].tobytes()


def at_distance(d, x=LETTERS, tail=b"!?"):
    """text in which x repeats exactly d bytes behind itself.  d <= 4: d different bytes over and over.  Else x, a run of one
    byte (it is a single table entry, so x's own entry lives on; 32 K of random bytes would overwrite all 4096) and x."""
    if d <= 4:
        return (b"abcd"[:d] * 8)[:d + 20] + tail
    assert d >= len(x) + 1 and b"a" not in x
    return x + b"a" * (d - len(x)) + x + tail


def _collisions(count):
    """pairs of unequal 4-grams of lower-case letters with one hash, the first `count` in dictionary order of the second"""
    import itertools
    import deflate_model as dm
    seen, out = {}, []
    for g in itertools.product(b"bcdefghijklm", repeat=4):
        g = bytes(g)
        h = dm.hash4(g, 0)
        if h in seen and not set(seen[h]) & set(g):
            out.append((seen[h], g))
            if len(out) == count:
                return out
        seen.setdefault(h, g)
    raise AssertionError("no collisions found")


def _tuned(rng, n, bits):
    """n random bytes whose fixed-code form has exactly `bits` bits: bytes below 144 (8 bits each), as many of them lifted to
    144 and above (9 bits) as it takes; the model counts, since a chance match changes the sum"""
    import deflate_model as dm
    base = _rand(rng, n, 0, 144)
    places = [int(q) for q in rng.permutation(n)]
    k = max(0, bits - (10 + 8 * n))  # (3 bits of header, 7 of end code, 8 a byte: what is missing without a match)
    for _ in range(10):
        t = bytearray(base)
        for q in places[:k]:
            t[q] = 144 + base[q] % 112
        have = dm.fixed_bits(dm.tokens(t))
        if have == bits:
            return bytes(t)
        k += bits - have
        assert 0 <= k <= n
    raise AssertionError("no block of %d bytes with %d bits" % (n, bits))


def edge_corpus():
    """[(name, [blocks])], every block 1 .. 0xff00 bytes"""
    import deflate_model as dm
    rng = np.random.default_rng(23)
    out = []
    x12 = b"klmnopqrstuv"

    # the window: distance 32768 is the last that may be coded, 32769 must be refused (at every byte of x: the repeat of 12
    # bytes offers it nine times)
    out.append(("window", [at_distance(d, x, tail) for d in (32767, 32768, 32769) for x, tail in ((LETTERS, b"!?"), (LETTERS, b""), (x12, b"!?"))]))
    bounds = sorted(set(dm.DIST_BASE + [b - 1 for b in dm.DIST_BASE[1:]] + [dm.WINDOW]))
    out.append(("distance_codes", [at_distance(d) for d in bounds] + [at_distance(d, x12) for d in bounds if 12 < d <= 4097]))

    # every length, at distances 1 .. 4 (cut by the block's end, and by a byte that differs), at its own length (a string
    # of bytes >= 144 twice), far back and at the window's bound; longer than 258: 258 and the rest
    lengths = list(range(4, 263)) + [300, 515, 516, 517, 518, 519, 520, 600]
    blocks = []
    for d in (1, 2, 3, 4):
        for L in lengths:
            t = (b"abcd"[:d] * (L // d + 2))[:d + L]
            blocks += [t, t + b"\x00\x01\x02\x03"]
    out.append(("lengths_near", blocks))
    blocks = []
    for L in lengths:
        r = _rand(rng, L, 144, 256)
        blocks.append(r + r + b"\x00\x01")
    out.append(("lengths_doubled", blocks))
    blocks = []
    for L in range(4, 259):
        r = _rand(rng, L, 32, 97)
        blocks.append(r + b"a" * 300 + r + b"\x00")
    for L in (4, 227, 257, 258, 259):
        r = _rand(rng, L, 32, 97)
        blocks.append(r + b"a" * (32768 - L) + r + b"\x00")
    out.append(("lengths_far", blocks))

    # 9-bit literals beside matches: words and single bytes of 144 .. 255
    words = [_rand(rng, int(k), 144, 256) for k in rng.integers(3, 10, 40)]
    text = b"".join(words[int(rng.integers(40))] if rng.random() < 0.6 else _rand(rng, 2, 144, 256) for _ in range(6000))
    out.append(("high_literals", [text[at:at + 8000] for at in range(0, 24000, 8000)]))

    # stored or fixed: n different bytes >= 144 take 10 + 9 n bits, so the fixed form falls behind the stored form's 5 + n
    # bytes as n grows; the same with a repeat among them; and blocks of the largest sizes tuned to the last bit at which
    # fixed wins, the first and the last of the tie, and the first at which it is larger
    perm = _distinct(rng, 112, 144, 256)
    blocks = [perm[:n] for n in range(1, 41)] + [perm[:m] + perm[:6] for m in range(20, 61)]
    n = MAX_BLOCK
    blocks += [_tuned(rng, n, b) for b in (8 * (n + 4), 8 * (n + 4) + 1, 8 * (n + 5), 8 * (n + 5) + 1)]
    blocks += [_tuned(rng, n - 1, b) for b in (8 * (n + 3), 8 * (n + 3) + 1)]
    out.append(("stored_or_fixed", blocks))

    # the schedule of 64 positions a step.  One tail text behind 0 .. 63 (and 62 .. 66, 126 .. 130) leading bytes that occur
    # nowhere else, so that every event below falls on every place of a step and across every step's end:
    #   wxyz three times within 23 bytes: the third must take the second, not the first;
    #   wxyz twice more 70 bytes on: the second has one candidate in the table and, in most blocks, one in its own step;
    #   330 times one byte: one hash on all 64 positions of a step, matches of 258 that pass whole steps;
    #   300 random bytes, then their first 258 again (a match that passes three steps in most blocks) and at once bytes
    #   100 .. 140 of them: their latest occurrence lies inside the match just taken, 158 back, where only the table went.
    v = _rand(rng, 300, 32, 97)
    tail = (b"wxyz" + b"ABC" + b"wxyz" + b"DEFGH" + b"wxyz" + b"IJ" + bytes(range(219, 149, -1)) + b"wxyz" + b"KLMNOP" + b"wxyz" + b"QR" +
            b"a" * 330 + b"ST" + v + b"UV" + v[:258] + v[100:140] + b"WX")
    out.append(("schedule", [bytes(range(1, 1 + k)) + tail for k in range(64)] +
                [bytes(range(123, 123 + k)) + tail for k in (62, 63, 64, 65, 66, 126, 127, 128, 129, 130)]))

    # two unequal 4-grams with one hash: g2 takes g1's table entry, so g1's true repeat is not found and is written as
    # literals; with other bytes in g2's place it is found (the same blocks with the repeat five bytes longer, and with g2 a
    # step or more away)
    blocks = []
    for g1, g2 in _collisions(5):
        for between in (g2, b"GHIJ"):
            for more in (b"", b"nopqr"):
                for gap in (b"", bytes(range(0, 48)) + bytes(range(75, 98)) + bytes(range(115, 144))):
                    blocks.append(b"0123" + g1 + more + b"4567" + between + gap + b"89AB" + g1 + more + b"CDEF")
    out.append(("collisions", blocks))

    # ends: a match that the block's end cuts at 1 .. 5, 257, 258 bytes; blocks too short for a hash or a match; a block of
    # the largest size whose last 258 bytes are one match
    r = _rand(rng, 258, 32, 97)
    blocks = [r + b"a" * 50 + r[:k] for k in (1, 2, 3, 4, 5, 256, 257, 258)]
    for n in range(1, 8):
        blocks += [b"a" * n, b"abcdefg"[:n], b"abababa"[:n], b"abcabca"[:n], bytes([200]) * n, bytes(range(250, 250 - n, -1))]
    blocks.append(b"b" * (MAX_BLOCK - 2 * 258 - 20000) + r + b"a" * 20000 + r)
    out.append(("ends", blocks))

    # random text of 2, 3 and 4 letters: many candidates a hash, short and long matches at every distance
    blocks = []
    for letters in (b"ab", b"abc", b"abcd", bytes([200, 201, 202])):
        lut = np.frombuffer(letters, np.uint8)
        blocks += [lut[rng.integers(0, len(letters), 3000)].tobytes() for _ in range(3)]
        if letters in (b"ab", b"abcd"):
            blocks.append(lut[rng.integers(0, len(letters), MAX_BLOCK)].tobytes())
    out.append(("few_letters", blocks))

    for name, blocks in out:
        assert all(1 <= len(b) <= MAX_BLOCK for b in blocks), name
    return out


def edge_text(edge):
    """the edge corpus as one text and its block sizes"""
    blocks = [b for _, bs in edge for b in bs]
    return b"".join(blocks), [len(b) for b in blocks]


_traces = {}


def traced(m):
    """the tracer's reading of a member's payload (kept by the member's bytes: the same bytes read the same)"""
    import deflate_writer as dw
    if m not in _traces:
        _traces[m] = dw.trace(m[18:-8])
    return _traces[m]


def edge_report(members, blocks):
    """what the tracer finds in the members of the edge corpus"""
    import deflate_model as dm
    import deflate_writer as dw
    rep = dict(lengths=set(), distances=set(), distance_codes=set(), high_literals_beside_matches=0, stored=0, ties=0, split_258=0)
    for m, block in zip(members, blocks):
        tr = traced(m)
        assert tr.text == block and len(tr.blocks) == 1
        if tr.blocks[0][0] == 0:
            rep["stored"] += 1
            # a tie: this text's tokens, counted with the code lengths of tests/deflate_writer.py, take the stored form's bytes
            bits = 3 + 7
            for t in dm.tokens(block):
                if isinstance(t, int):
                    bits += dw.FIXED_LIT_LENS[t]
                else:
                    (ls, le, _), (_, de, _) = dw.length_symbol(t[0]), dw.distance_symbol(t[1])
                    bits += dw.FIXED_LIT_LENS[ls] + le + 5 + de
            rep["ties"] += (bits + 7) // 8 == 5 + len(block)
            continue
        matches = [t for t in tr.tokens if not isinstance(t, int)]
        rep["lengths"] |= {t[0] for t in matches}
        rep["distances"] |= {t[1] for t in matches}
        rep["distance_codes"] |= {dw.distance_symbol(t[1])[0] for t in matches}
        rep["split_258"] += any(a[0] == 258 and not isinstance(b, int) and a[1] == b[1] for a, b in zip(tr.tokens, tr.tokens[1:]) if not isinstance(a, int))
        if matches:
            rep["high_literals_beside_matches"] += sum(1 for t in tr.tokens if isinstance(t, int) and t >= 144)
    return rep


def assert_edge_conditions(rep):
    """the conditions on the edge corpus: where the members must have gone, whoever wrote them"""
    assert rep["lengths"] == set(range(4, 259)), sorted(set(range(4, 259)) ^ rep["lengths"])
    assert rep["distance_codes"] == set(range(30)), sorted(rep["distance_codes"])
    assert {1, 2, 3, 4, 32767, 32768} <= rep["distances"] and max(rep["distances"]) == 32768
    assert rep["high_literals_beside_matches"] > 1000, rep["high_literals_beside_matches"]
    assert rep["ties"] >= 1 and rep["stored"] > rep["ties"] and rep["split_258"] >= 1, rep


def cpu_members(core_exe, text, sizes, work_dir, sanitize_env=True, level="fast"):
    """the CPU build of the core (tests/cpp/deflate_core_check.cpp) over the blocks at the level: the members, back to back"""
    tp, op, sp = (os.path.join(str(work_dir), n) for n in ("text.bin", "members.bin", "sizes.txt"))
    with open(tp, "wb") as fh:
        fh.write(text)
    with open(sp, "w") as fh:
        fh.write("\n".join(str(s) for s in sizes) + "\n")
    p = subprocess.run([core_exe, "--level", level, tp, op, "@" + sp], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV), timeout=1200)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    with open(op, "rb") as fh:
        return fh.read()


def first_difference(got, want):
    """where two members of one text part, in the tracer's tokens"""
    try:
        a, b = traced(got).tokens, traced(want).tokens
    except Exception as e:  # (not a stream at all)
        return "the tracer: %r" % (e,)
    at = 0
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "token %d, at byte %d of the text: the encoder wrote %r, the model %r" % (k, at, x, y)
        at += 1 if isinstance(x, int) else x[0]
    if len(a) != len(b):
        return "%d tokens against the model's %d" % (len(a), len(b))
    return "the same tokens; member bytes %d against %d, first difference at byte %d" % (
        len(got), len(want), next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want))))


def assert_members_are_the_models(names, members, expected):
    bad = [(name, first_difference(m, e)) for name, m, e in zip(names, members, expected) if m != e]
    assert not bad, "%d of %d members differ from the model's; the first: %s: %s" % (len(bad), len(members), bad[0][0], bad[0][1])


def offsets(sizes):
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    return off


def assert_members(got, want, sizes, what):
    """the members back to back against the expected ones; on a difference, the first block that differs"""
    if got == want:
        return
    a, b = split_members(got), split_members(want)
    k = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    raise AssertionError("%s: %d members against %d; the first difference is block %d of %d bytes (%d bytes against %d)" % (
        what, len(a), len(b), k, sizes[k] if k < len(sizes) else -1, len(a[k]) if k < len(a) else -1, len(b[k]) if k < len(b) else -1))


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
