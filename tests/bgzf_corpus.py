"""The corpus of BGZF members that the device DEFLATE decoder is held to (tests/test_bgzf_cpu.py through the CPU build of
basevar_amd/csrc/bv_inflate_core.h, tests/test_gpu_bgzf.py on the GPU): valid members made at run time with zlib over every
block type, level and strategy, and damaged variants, each made from a valid member or bit by bit.  zlib is the oracle."""
import os
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_HEADER, BAD_DEFLATE, BAD_SIZE, BAD_CRC = 0, 1, 2, 3, 4
HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"


def wrap(payload, data=None, crc=None, isize=None, bsize=None):
    """a raw DEFLATE payload as one BGZF member (SAM specification 4.1)"""
    total = 18 + len(payload) + 8
    crc = (zlib.crc32(data) & 0xFFFFFFFF) if crc is None else crc
    isize = len(data) if isize is None else isize
    return HEAD + struct.pack("<H", (total - 1 if bsize is None else bsize) & 0xFFFF) + bytes(payload) + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """raw DEFLATE of data; flushes = [(offset, zlib flush mode)]: the stream is flushed that way at those offsets"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out, at = b"", 0
    for off, mode in flushes:
        out += co.compress(data[at:off]) + co.flush(mode)
        at = off
    return out + co.compress(data[at:]) + co.flush()


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    m = wrap(deflate(data, level, strategy, flushes), data)
    assert len(m) <= 65536, "not a BGZF member: %d bytes" % len(m)
    return m


def payload_of(m):
    return m[18:-8]


def rows_text(n_bytes, seed=3, samples=200):
    """batchfile rows in the reference's format (the generator of tests/test_gpu_text_rows.py), the first n_bytes of them"""
    from basevar_amd.synth import make_slab
    from test_gpu_text_rows import slab_rows
    slab = make_slab(max(2, n_bytes // (samples * 3) + 2), samples, seed=seed, coverage=0.08)
    text, _ = slab_rows(slab, [samples])
    assert text.size >= n_bytes
    return text[:n_bytes].tobytes()


def contents():
    rng = np.random.default_rng(11)
    return [("rows", rows_text(0xff00)), ("rows64k", rows_text(65536, seed=4)), ("rows_short", rows_text(700, seed=5)),
            ("random", rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()), ("one_byte_repeated", b"a" * 30000),
            ("period3", b"xyz" * 7000), ("empty", b""), ("single", b"Q"), ("rows65280", rows_text(65280, seed=6))]


def valid_corpus():
    """[(name, member bytes, inflated bytes)]"""
    out = []
    strategies = [("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE),
                  ("filtered", zlib.Z_FILTERED)]
    for cname, data in contents():
        for level in (0, 1, 6, 9):
            for sname, strat in strategies:
                if level == 0 and sname != "default":
                    continue
                # (stored: the payload is longer than its text, and a member holds 64 KiB in all)
                data_ = data[:65280] if level == 0 else data
                out.append(("%s/l%d/%s" % (cname, level, sname), member(data_, level, strat), data_))
        if len(data) >= 700:
            third = len(data) // 3
            cut = data[:60000]
            out.append((cname + "/full_flush", member(cut, 6, flushes=[(third, zlib.Z_FULL_FLUSH)]), cut))
            out.append((cname + "/sync_flush", member(cut, 1, flushes=[(third, zlib.Z_SYNC_FLUSH), (2 * third, zlib.Z_SYNC_FLUSH)]), cut))
            out.append((cname + "/fixed_then_dynamic", wrap(_two_streams(cut, third), cut), cut))
    return out


def _two_streams(data, cut):
    """data[:cut] as fixed-Huffman blocks, the rest as whatever level 6 chooses: one stream with several block types"""
    a = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    first = a.compress(data[:cut]) + a.flush(zlib.Z_FULL_FLUSH)  # ends on a byte boundary with an empty stored block, not final
    return first + deflate(data[cut:], 6)


class Bits:
    """DEFLATE's bit order: values from the low bit up, Huffman codes from their first bit"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        return self

    def code(self, code, nbits):
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)
        return self

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _fixed_lit(b, sym):
    if sym < 144:
        return b.code(0x30 + sym, 8)
    if sym < 256:
        return b.code(0x190 + sym - 144, 9)
    if sym < 280:
        return b.code(sym - 256, 7)
    return b.code(0xC0 + sym - 280, 8)


def _canonical(lens):
    code, out = 0, {}
    for l in range(1, 16):
        for s, x in enumerate(lens):
            if x == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_header(cl_lens, items, hlit, hdist, final=1):
    """a dynamic block's header: cl_lens {symbol of the code-length code: its length}, items [(cl symbol, extra value)]"""
    b = Bits().put(final, 1).put(2, 2).put(hlit, 5).put(hdist, 5)
    last = max(CL_ORDER.index(s) for s in cl_lens) if cl_lens else 3
    b.put(max(last + 1, 4) - 4, 4)
    for s in CL_ORDER[:max(last + 1, 4)]:
        b.put(cl_lens.get(s, 0), 3)
    codes = _canonical([cl_lens.get(s, 0) for s in range(19)])
    for s, extra in items:
        c, l = codes[s]
        b.code(c, l)
        if s >= 16:
            b.put(extra, {16: 2, 17: 3, 18: 7}[s])
    return b


def crafted():
    """[(name, member)] built bit by bit; zlib decides what each one is"""
    out = []

    def add(name, bits, data=b""):
        out.append((name, wrap(bits.bytes() if isinstance(bits, Bits) else bits, data)))
    # a first match that reaches before the member's first byte: literal 'a', then length 3 at distance 2
    add("distance_too_far", _fixed_lit(_fixed_lit(Bits().put(1, 1).put(1, 2), 97), 257).code(1, 5), b"aaaa")
    # ... and the same match at distance 1: valid ("aaaa")
    add("distance_ok", _fixed_lit(_fixed_lit(_fixed_lit(Bits().put(1, 1).put(1, 2), 97), 257).code(0, 5), 256), b"aaaa")
    add("fixed_symbol_286", _fixed_lit(_fixed_lit(Bits().put(1, 1).put(1, 2), 97), 286), b"a")
    add("fixed_distance_30", _fixed_lit(_fixed_lit(Bits().put(1, 1).put(1, 2), 97), 257).code(30, 5), b"aaaa")
    add("btype3", Bits().put(1, 1).put(3, 2).put(0, 13))
    add("stored_len_nlen", Bits().put(1, 1).put(0, 2).put(0, 5).put(3, 16).put(0xFFFC ^ 0x10, 16).put(0x636261, 24), b"abc")
    add("stored_ok", Bits().put(1, 1).put(0, 2).put(0, 5).put(3, 16).put(0xFFFC, 16).put(0x636261, 24), b"abc")
    add("hlit_287", Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).put(0, 40))
    add("hdist_31", Bits().put(1, 1).put(2, 2).put(0, 5).put(30, 5).put(0, 4).put(0, 40))
    add("cl_oversubscribed", dynamic_header({0: 1, 1: 1, 2: 1}, [], 0, 0).put(0, 64))
    add("cl_incomplete", dynamic_header({0: 1}, [], 0, 0).put(0, 64))
    add("cl_all_zero", dynamic_header({}, [], 0, 0).put(0, 300))
    # 257 literal/length codes of one bit: over-subscribed
    add("lit_oversubscribed", dynamic_header({1: 1, 18: 1}, [(1, 0)] * 257 + [(1, 0)], 0, 0).put(0, 32))
    # two codes of two bits (symbols 0 and 256): incomplete, and longer than one bit
    add("lit_incomplete", dynamic_header({2: 1, 18: 2, 0: 2}, [(2, 0), (18, 127), (18, 106), (2, 0), (0, 0)], 0, 0).put(0, 32))
    # only symbol 256, one bit: incomplete and accepted; the block is its end code
    only_eob = [(18, 127), (18, 107), (1, 0), (0, 0)]
    add("only_end_of_block", dynamic_header({1: 1, 18: 2, 0: 2}, only_eob, 0, 0).put(0, 1))
    add("only_end_of_block_then_no_code", dynamic_header({1: 1, 18: 2, 0: 2}, only_eob, 0, 0).put(1, 1).put(0, 16))
    # two literal codes (symbols 97 and 256), no distance code at all, and a length symbol cannot be written: valid "aa"
    two = [(18, 86), (1, 0), (18, 127), (18, 9), (1, 0), (0, 0)]
    add("no_distance_codes", dynamic_header({1: 1, 18: 2, 0: 2}, two, 0, 0).put(0, 1).put(0, 1).put(1, 1), b"aa")
    add("repeat_without_previous", dynamic_header({16: 1, 1: 1}, [(16, 0)], 0, 0).put(0, 32))
    add("repeat_past_the_end", dynamic_header({18: 1, 1: 1}, [(18, 127), (18, 127)], 0, 0).put(0, 32))
    add("no_end_of_block_code", dynamic_header({1: 1, 18: 2, 0: 2}, [(1, 0), (1, 0), (18, 127), (18, 106), (0, 0)], 0, 0).put(0, 32))
    return out


def damaged_corpus(seed=29):
    """[(name, member)]: variants of valid members; a variant may be valid by chance and zlib says so"""
    rng = np.random.default_rng(seed)
    out = list(crafted())
    valid = {n: (m, d) for n, m, d in valid_corpus()}
    bases = ["rows/l1/default", "rows/l6/default", "rows_short/l9/fixed", "rows_short/l0/default", "random/l6/default", "one_byte_repeated/l6/rle",
             "period3/l1/default", "rows/sync_flush", "rows/fixed_then_dynamic", "single/l6/default", "empty/l6/default", "rows64k/l6/default"]
    for name in bases:
        m, data = valid[name]
        p = payload_of(m)
        cuts = sorted(set([0, 1, 2, 5, len(p) // 2, len(p) - 1] + [int(x) for x in rng.integers(0, max(1, len(p)), 6)]))
        for c in cuts:
            if 0 <= c < len(p):
                out.append(("%s/cut%d" % (name, c), wrap(p[:c], data)))
        for k in range(12):
            q = bytearray(p)
            if not q:
                break
            # early bits (the block header, the code lengths) as often as anywhere
            i = int(rng.integers(0, min(len(q), 40))) if k % 2 else int(rng.integers(0, len(q)))
            q[i] ^= 1 << int(rng.integers(0, 8))
            out.append(("%s/flip%d" % (name, k), wrap(q, data)))
        out.append((name + "/isize+1", wrap(p, data, isize=len(data) + 1)))
        if data:
            out.append((name + "/isize-1", wrap(p, data, isize=len(data) - 1)))
        out.append((name + "/crc", wrap(p, data, crc=zlib.crc32(data) ^ 0x00100000)))
        if p:
            out.append((name + "/btype3", wrap(bytes([p[0] | 0x06]) + p[1:], data)))
        out.append((name + "/bsize+1", wrap(p, data, bsize=18 + len(p) + 8)))
        out.append((name + "/bsize-1", wrap(p, data, bsize=18 + len(p) + 8 - 2)))
        out.append((name + "/magic", b"\x1f\x8c" + m[2:]))
        out.append((name + "/no_bc", m[:12] + b"XY" + m[14:]))
        out.append((name + "/isize_huge", wrap(p, data, isize=len(data) + 0x10000)))
    m, data = valid["rows_short/l0/default"]
    q = bytearray(payload_of(m))
    q[3] ^= 0x01  # NLEN of the stored block
    out.append(("rows_short/l0/nlen", wrap(q, data)))
    return out


def pack(members):
    """(bytes, member_off uint64 [n + 1]) of the members one behind the other, as they lie in a file"""
    off = np.zeros(len(members) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in members])
    return b"".join(members), off


def write_corpus(path, members):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(members)))
        for m in members:
            fh.write(struct.pack("<I", len(m)) + m)


def build_core_check(out_dir, sanitize=False):
    """tests/cpp/inflate_core_check.cpp compiled with g++ (plain, or ASan + UBSan)"""
    exe = os.path.join(str(out_dir), "inflate_core_check" + (".asan" if sanitize else ""))
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "inflate_core_check.cpp"), "-lz", "-o", exe])
    return exe


def core_verdicts(exe, members, work_dir):
    """run the CPU build of the core on the members: (CompletedProcess, [(core status, zlib status, block mask, isize)])"""
    path = os.path.join(str(work_dir), "corpus.bin")
    write_corpus(path, members)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    p = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    rows = [tuple(int(x) for x in line.split()[1:]) for line in p.stdout.splitlines() if line.strip()]
    return p, rows


def assert_block_coverage(names, members, verdicts):
    """the valid corpus holds a stored, a fixed and a dynamic first block and a member with more than one block type"""
    first = {(payload_of(m)[0] >> 1) & 3 for m in members if payload_of(m)}
    assert {0, 1, 2} <= first, first
    mixed = [n for n, v in zip(names, verdicts) if bin(v[2]).count("1") > 1]
    assert mixed, "no member with more than one block type"
    return mixed
