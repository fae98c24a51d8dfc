"""The corpus of BGZF members that the device DEFLATE decoder is held to (tests/test_bgzf_cpu.py through the CPU build of
basevar_amd/csrc/bv_inflate_core.h, tests/test_gpu_bgzf.py on the GPU): valid members made at run time with zlib over every
block type, level and strategy, and damaged variants, each made from a valid member or bit by bit; and a foreign corpus
(foreign_corpus(), foreign_damaged()) of members that zlib inflates and its compressor never writes, encoded by
tests/deflate_writer.py.  zlib is the oracle."""
import os
import struct
import subprocess
import zlib
from collections import Counter

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


# ---------------------------------------------------------------------------------------------------------------------------
# The foreign corpus: members that zlib's inflate accepts and zlib's deflate never writes, encoded by tests/deflate_writer.py.
# zlib judges every one (zlib.decompress(payload, -15) gives the bytes); deflate_writer.trace says which features each holds.

FOREIGN_SIZES = list(range(0, 50)) + [k * 1024 + d for k in (1, 2, 63) for d in (-1, 0, 1)] + [65535, 65536]


def wrap_gzip(payload, data, subfields=(("BC", None),), flg=4, mtime=0, xfl=0, os_=255, fname=None, hcrc=False, crc=None, isize=None):
    """a gzip member (RFC 1952) around the payload: subfields [(two-letter id, bytes)]; the bytes None stand for the BGZF length"""
    extra_len = sum(4 + (2 if b is None else len(b)) for _, b in subfields)
    tail = (fname + b"\0" if fname is not None else b"") + (b"\0\0" if hcrc else b"")
    total = 12 + extra_len + len(tail) + len(payload) + 8
    extra = b"".join(i.encode() + struct.pack("<H", 2 if b is None else len(b)) + (struct.pack("<H", (total - 1) & 0xFFFF) if b is None else b)
                     for i, b in subfields)
    head = b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<IBBH", mtime, xfl, os_, extra_len) + extra
    if fname is not None:
        head += fname + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    crc = (zlib.crc32(data) & 0xFFFFFFFF) if crc is None else crc
    return head + bytes(payload) + struct.pack("<II", crc, len(data) if isize is None else isize)


class _Tok:
    """a token list under construction and the text it stands for"""

    def __init__(self):
        self.t, self.out, self.taken = [], bytearray(), 0

    def lit(self, *bs):
        for b in bs:
            self.t.append(int(b))
            self.out.append(int(b))
        return self

    def match(self, length, dist, alt=False):
        assert 1 <= dist <= len(self.out) and 3 <= length <= 258
        self.t.append((length, dist, True) if alt else (length, dist))
        for _ in range(length):
            self.out.append(self.out[-dist])
        return self

    def fill_to(self, n, dists):
        """matches of 258 bytes at the distances in turn (where they reach), and a shorter one or two, up to byte n exactly"""
        k = 0
        while n - len(self.out) >= 3:
            r = n - len(self.out)
            length = 258 if r >= 261 else r if r <= 258 else r - 3
            d = dists[k % len(dists)]
            k += 1
            self.match(length, d if d <= len(self.out) else 1)
        while len(self.out) < n:
            self.lit(0x21 + len(self.out) % 90)
        assert len(self.out) == n
        return self

    def take(self):
        """the tokens added since the last take()"""
        part, self.taken = self.t[self.taken:], len(self.t)
        return part


def _random_tokens(rng, tok, size):
    while len(tok.out) < size:
        r = size - len(tok.out)
        if r >= 3 and tok.out and rng.random() < 0.5:
            far = min(len(tok.out), 32768)
            dist = int(rng.integers(1, far + 1)) if rng.random() < 0.5 else int(rng.integers(1, min(far, 40) + 1))
            tok.match(int(min(r, rng.integers(3, 259))), dist)
        else:
            tok.lit(int(rng.integers(0, 256)) if rng.random() < 0.3 else int(rng.integers(97, 105)))
    return tok


_FOREIGN = {}


def _foreign():
    """[(name, member, data, blocks)]; data is zlib's inflation of the payload"""
    if "valid" in _FOREIGN:
        return _FOREIGN["valid"]
    import deflate_writer as dw
    out = []

    def add(name, blocks, gzip=None, **kw):
        payload = dw.write_stream(blocks, **kw)
        data = zlib.decompress(payload, -15)  # the judge
        m = wrap(payload, data) if gzip is None else wrap_gzip(payload, data, **gzip)
        assert len(m) <= 65536, (name, len(m))
        out.append((name, m, data, blocks))

    def dyn(tokens, **kw):
        return dict({"type": "dynamic", "tokens": tokens}, **kw)

    def fixed(tokens, **kw):
        return dict({"type": "fixed", "tokens": tokens}, **kw)

    def stored(data, **kw):
        return dict({"type": "stored", "data": bytes(data)}, **kw)

    rng = np.random.default_rng(101)
    az = list(range(97, 111))  # 14 literals
    lit16 = dw.assign(az + [257, 256], dw.skewed_lengths(16, 15), 286)
    dist16 = dw.assign(list(range(16)), dw.skewed_lengths(16, 15), 30)

    # every code length 1 .. 15 of both alphabets decoded: 16 symbols each, lengths 1, 2, ..., 15, 15, every symbol used
    t = _Tok().lit(*[az[k % 14] for k in range(200)])
    for s in range(16):
        t.match(3, dw.DIST_BASE[s])
    add("lengths_1_to_15", [dyn(t.take(), lit_lens=lit16, dist_lens=dist16)])
    # ... and with the long codes on the other end of each alphabet
    t = _Tok().lit(*[az[k % 14] for k in range(200)])
    for s in range(16):
        t.match(3, dw.DIST_BASE[s])
    add("lengths_15_to_1", [dyn(t.take(), lit_lens=dw.assign([256, 257] + az[::-1], dw.skewed_lengths(16, 15), 286),
                                dist_lens=dw.assign(list(range(15, -1, -1)), dw.skewed_lengths(16, 15), 30), spell="plain")])

    # everything at once: 65 536 bytes, all 286 + 30 symbols coded, 15-bit codes in both alphabets, every length and distance
    # symbol with its smallest and largest extra bits, distance 32 768 from the first byte it is legal at
    lengths = [(dw.LEN_BASE[s] + e, s == 27 and e > 0) for s in range(28) for e in sorted({0, (1 << dw.LEN_EXTRA[s]) - 1})] + [(258, False)]
    dists = [dw.DIST_BASE[s] + e for s in range(30) for e in sorted({0, (1 << dw.DIST_EXTRA[s]) - 1})]
    near = [1, 2, 3, 7, 63, 64, 65, 257, 5, 1000, 31, 258]
    t = _Tok().lit(*rng.permutation(256)).lit(*rng.integers(0, 256, 6000))
    k = 0
    for length, alt in lengths:
        for _ in range(2):
            d = [x for x in dists if x <= len(t.out)]
            t.lit(int(rng.integers(0, 256))).match(length, d[k % len(d)], alt)
            k += 1
    for d in (3, 4, 16, 64, 100, 258):  # the source ends on the literal just written
        t.lit(0x41 + d % 26).match(d, d)
    t.fill_to(32768, near)
    t.match(258, 32768)
    for k, d in enumerate(dists + [32507, 32600, 32767, 32768]):
        t.lit(int(rng.integers(0, 256))).match(*((lengths[k % len(lengths)][0], d) + ((True,) if lengths[k % len(lengths)][1] else ())))
    t.fill_to(65536 - 258, near + [32768, 32767, 32507, 20000])
    t.match(258, 32768, True)
    assert len(t.out) == 65536
    tokens = t.take()
    lit_used, dist_used = dw._used(tokens)
    lit_syms = [s for s, _ in sorted(lit_used.items(), key=lambda kv: (-kv[1], kv[0]))]
    dist_syms = [s for s, _ in sorted(dist_used.items(), key=lambda kv: (-kv[1], kv[0]))]
    assert len(lit_syms) == 286 and len(dist_syms) == 30
    every = dict(lit_lens=dw.assign(lit_syms, dw.skewed_lengths(286, 15), 286), dist_lens=dw.assign(dist_syms, dw.skewed_lengths(30, 15), 30))
    seq = every["lit_lens"] + every["dist_lens"]
    cl_syms = [s for s, _ in Counter(o if isinstance(o, int) else int(o[0][1:]) for o in dw.spell_lengths(seq, "rle")).most_common()]
    cl7 = dict(zip(cl_syms, dw.skewed_lengths(len(cl_syms), 7)))
    add("everything_at_once", [dyn(tokens, cl_lens=cl7, hclen=19, **every)])
    add("everything_in_blocks", [dyn(tokens[lo:lo + 500], spell="plain", **every) for lo in range(0, len(tokens), 500)])

    # overlapping matches, the earliest legal source at distance 1, sources that end on the literal before the match
    t = _Tok().lit(0x78).match(258, 1).lit(*rng.integers(0, 256, 300))
    for d in (1, 2, 3, 7, 63, 64, 65):
        t.match(258, d).lit(int(rng.integers(0, 256))).match(d + 1 if d >= 2 else 3, d).lit(int(rng.integers(0, 256)))
    t.match(258, 257)
    for d in (3, 4, 16, 64, 100, 258):
        t.lit(0x41 + d % 26).match(d, d)
    tokens = t.take()
    add("overlaps/fixed", [fixed(tokens)])
    add("overlaps/dynamic", [dyn(tokens)])
    lit_used, dist_used = dw._used(tokens)
    add("overlaps/skewed", [dyn(tokens, lit_lens=dw.assign(*dw.by_frequency(lit_used, lambda n: dw.skewed_lengths(n, 15)), 286),
                                dist_lens=dw.assign(*dw.by_frequency(dist_used, lambda n: dw.skewed_lengths(n, min(15, n - 1))), 30))])

    # headers.  HCLEN 4 gives lengths to the symbols 16, 17, 18 and 0 only: every code length is then 0 and no block is valid,
    # so the smallest HCLEN of a valid block is 5 (symbol 8); HCLEN 4 is in foreign_damaged().
    add("header/hlit257_hdist1_hclen5", [dyn([0, 7, 254, 256 - 2], lit_lens=[8] * 255 + [0, 8], dist_lens=[0], spell="plain")])
    lens = [4] * 11 + [0] * 3 + [4] + [0] * 10 + [4] + [0] * 11 + [4] + [0] * 138 + [4] + [0] * 79 + [4]
    add("header/repeat_counts", [dyn([0, 5, 14, 25, 37, 176], lit_lens=lens, dist_lens=[0],
                                     spell=[4, ("r16", 3), 4, ("r16", 6), ("r17", 3), 4, ("r17", 10), 4, ("r18", 11), 4, ("r18", 138), 4, ("r18", 79), 4, 0])])
    add("header/repeat_16_crosses", [dyn([254, 255, (3, 1), (3, 2), (3, 3), (3, 4)], lit_lens=[0] * 254 + [2] * 4, dist_lens=[2] * 4,
                                         spell=[("r18", 138), ("r18", 116), 2, ("r16", 6), 2])])
    two = [0] * 97 + [2, 2] + [0] * 157 + [2, 2]
    add("header/repeat_17_crosses", [dyn([97, 98, 97, 98, (3, 4)], lit_lens=two, dist_lens=[0, 0, 0, 1], hlit=260,
                                         spell=[("r18", 97), 2, 2, ("r18", 138), ("r18", 19), 2, 2, ("r17", 5), 1])])
    add("header/repeat_18_crosses", [dyn([97, 98] * 30 + [(3, 33), (3, 48)], lit_lens=two, dist_lens=[0] * 10 + [1], hlit=270,
                                         spell=[("r18", 97), 2, 2, ("r18", 138), ("r18", 19), 2, 2, ("r18", 22), 1])])
    add("header/one_distance_code_used", [dyn([97, (3, 1), (3, 1)], lit_lens=dw.assign([257, 97, 256], [1, 2, 2], 286), dist_lens=[1])])
    only_end = dyn([], lit_lens=[0] * 256 + [1], dist_lens=[0])
    add("header/only_end_code_then_fixed", [only_end, fixed([104, 105])])
    add("header/only_end_code_alone", [only_end])

    # stored blocks
    add("stored/len0_first_middle_final", [stored(b""), fixed([97, 98, (3, 2)]), stored(b"", pad=1), fixed([99]), stored(b"", pad=1)])
    add("stored/len0_alone", [stored(b"")])
    add("stored/65505", [stored(rng.integers(0, 256, 65505, dtype=np.uint8).tobytes())])
    blocks = []
    for k in range(16):  # k literals of 9 bits move the end of the block through every bit of a byte
        blocks += [fixed([200] * k + [97, 98]), stored(rng.integers(0, 256, 2 * k + 1, dtype=np.uint8).tobytes(), pad=1)]
    add("stored/after_huffman_every_padding", blocks + [fixed([122])])
    add("stored/after_dynamic_every_padding", [b for k in range(8) for b in (dyn([200] * k + [97, 98, (4, 1)]), stored(bytes([65 + k]) * (k + 2), pad=1))]
        + [dyn([122])])

    # many blocks; code tables of very different depth one behind the other
    dyn15 = dict(lit_lens=lit16, dist_lens=[1, 1])
    dyn2 = dict(lit_lens=dw.assign([97, 98, 256, 257], [2] * 4, 286), dist_lens=[1, 1])
    blocks = []
    for k in range(334):
        blocks += [stored(bytes([48 + k % 10] * (1 + k % 5)), pad=k & 1), fixed([97 + k % 14, 98, (3 + k % 20, 1 + k % 2)]),
                   dyn([az[(k + j) % 14] for j in range(6)] + [(3, 2)], **dyn15) if k % 2 else dyn([97, 98, 98, (3, 1)], **dyn2)]
    add("thousand_blocks", blocks)
    add("deep_then_shallow_tables", [dyn(az + [(3, 1)], **dyn15), dyn([97, 98, (3, 2)], **dyn2), dyn(az[::-1] + [(3, 2)], **dyn15), fixed([97, (3, 1)]),
                                     dyn([98, 97], **dyn2)])

    # the end of the stream
    add("trailing_bytes_behind_the_final_block", [fixed([97, 98, 99])], trailing=b"\xff\xff\x00\x01 not deflate")
    add("final_block_ends_inside_a_byte/zeros", [fixed([97, 98, 99])], end_fill=0)

    # text sizes: the write-out's head / lines / tail split and the edges of the CRC slices
    for n in FOREIGN_SIZES:
        r = np.random.default_rng(1000 + n)
        t = _Tok()
        if n % 3 == 2:
            _random_tokens(r, t, n // 2)
            first = [stored(bytes(t.out), pad=1)]
            t.take()
        else:
            first = []
        _random_tokens(r, t, n)
        add("size/%d" % n, first + [fixed(t.take()) if n % 3 == 0 else dyn(t.take())])
    add("size/0/dynamic", [dyn([])])

    # the wrapper: what gzip allows around the BC subfield (judged by zlib.decompress(member, 31))
    t = _random_tokens(np.random.default_rng(77), _Tok(), 1500)
    blocks = [dyn(t.take())]
    for name, gz in (("extra_before_bc", dict(subfields=(("XY", b"abc"), ("BC", None)))), ("extra_behind_bc", dict(subfields=(("BC", None), ("ZZ", b"")))),
                     ("extra_on_both_sides", dict(subfields=(("AB", b"\0" * 9), ("BC", None), ("CB", b"BC\x02\x00")))),
                     ("mtime_xfl_os", dict(mtime=0x5F3759DF, xfl=2, os_=3)), ("xlen_300", dict(subfields=(("BC", None), ("PD", b"\x07" * 290))))):
        add("wrapper/" + name, blocks, gzip=gz)
        assert zlib.decompress(out[-1][1], 31) == out[-1][2]
    _FOREIGN["valid"] = out
    return out


def foreign_corpus():
    """[(name, member bytes, inflated bytes)]: valid members that zlib's own compressor does not write"""
    return [(n, m, d) for n, m, d, _ in _foreign()]


def foreign_blocks():
    """{name: the blocks the writer was given}"""
    return {n: b for n, _, _, b in _foreign()}


# gzip members that zlib reads and that are no BGZF members (SAM specification 4.1: FLG is FEXTRA alone, one BC subfield of 2 bytes)
GZIP_NOT_BGZF = {"wrapper/fname": "FLG has FNAME", "wrapper/fhcrc": "FLG has FHCRC", "wrapper/no_bc": "no BC subfield",
                 "wrapper/two_bc": "two BC subfields", "wrapper/bc_of_4_bytes": "a BC subfield of 4 bytes"}
# what zlib, asked for exactly ISIZE bytes, makes of the damaged members whose fault is known by construction
FOREIGN_DAMAGED_EXPECT = {}


def foreign_damaged():
    """[(name, member)]: damaged members made with the writer; zlib judges each (FOREIGN_DAMAGED_EXPECT: what it must find)"""
    if "damaged" in _FOREIGN:
        return _FOREIGN["damaged"]
    import deflate_writer as dw
    out = []
    rng = np.random.default_rng(202)

    def add(name, blocks, want, data=b"", isize=None, crc=None, cut=0, **kw):
        payload = blocks if isinstance(blocks, bytes) else dw.write_stream(blocks, **kw)
        out.append((name, wrap(payload[:len(payload) - cut], data, isize=isize, crc=crc)))
        FOREIGN_DAMAGED_EXPECT[name] = want

    def dyn(tokens, **kw):
        return dict({"type": "dynamic", "tokens": tokens, "check": False}, **kw)

    base = [int(x) for x in rng.integers(97, 123, 40)]
    for form, tail in (("distance_ge_length", (30, 35)), ("distance_1", (30, 1)), ("overlapping", (30, 7))):
        text = dw.expand(base + [tail])
        add("match_past_isize/" + form, [{"type": "fixed", "tokens": base + [tail]}], BAD_SIZE, text[:-9])
        add("match_past_isize/dynamic/" + form, [dyn(base + [tail], check=True)], BAD_SIZE, text[:-1])
    add("control/match_ends_on_isize", [{"type": "fixed", "tokens": base + [(30, 7)]}], OK, dw.expand(base + [(30, 7)]))
    add("distance_one_more_than_written", [{"type": "fixed", "tokens": base + [(5, 41), 97]}], BAD_DEFLATE, bytes(base) + b"aaaaaa")
    one = dict(lit_lens=dw.assign([257, 97, 256], [1, 2, 2], 286), dist_lens=[1])
    add("unassigned_code_of_a_one_code_distance_set", [dyn([97, ("sym", 257), ("bits", 1, 1), 97], **one)], BAD_DEFLATE, b"aaaaa")
    add("length_symbol_without_any_distance_code", [dyn([97, ("sym", 257), ("bits", 0, 8), 97], lit_lens=one["lit_lens"], dist_lens=[0])], BAD_DEFLATE, b"aaaaa")
    lens = [0] * 97 + [2, 2] + [0] * 157 + [2, 2]
    add("symbol_16_first", [dyn([97], lit_lens=lens, dist_lens=[0], spell=[("r16", 3)] + lens[3:] + [0])], BAD_DEFLATE, b"a")
    add("repeat_past_hlit_and_hdist_from_the_literal_part", [dyn([97], lit_lens=lens, dist_lens=[0], spell=[("r18", 97), 2, 2, ("r18", 138), ("r18", 138)])],
        BAD_DEFLATE, b"a")
    add("no_code_for_256_otherwise_complete", [dyn([97, 98, ("bits", 0, 16)], lit_lens=[0] * 97 + [1, 1], dist_lens=[0], hlit=257)], BAD_DEFLATE, b"ab")
    lit16 = dw.assign(list(range(97, 111)) + [257, 256], dw.skewed_lengths(16, 15), 286)
    dist16 = dw.assign(list(range(16)), dw.skewed_lengths(16, 15), 30)
    less = lambda lens: [0 if (l == 15 and k == max(i for i, x in enumerate(lens) if x == 15)) else l for k, l in enumerate(lens)]  # noqa: E731
    more = lambda lens, at: lens[:at] + [15] + lens[at + 1:]  # noqa: E731
    toks = [97, 98, 99, (3, 1)]
    add("incomplete_at_15_bits/literals", [dyn(toks[:3], lit_lens=less(lit16), dist_lens=dist16)], BAD_DEFLATE, b"abc")
    add("incomplete_at_15_bits/distances", [dyn(toks, lit_lens=lit16, dist_lens=less(dist16))], BAD_DEFLATE, b"abccc")
    add("oversubscribed_at_15_bits/literals", [dyn(toks, lit_lens=more(lit16, 5), dist_lens=dist16)], BAD_DEFLATE, b"abccc")
    add("oversubscribed_at_15_bits/distances", [dyn(toks, lit_lens=lit16, dist_lens=more(dist16, 20))], BAD_DEFLATE, b"abccc")
    add("hclen_4", [dyn([], lit_lens=[0] * 257, dist_lens=[0], cl_lens={0: 1, 18: 1}, spell=[("r18", 138), ("r18", 120)])], BAD_DEFLATE)
    add("stored_len_past_the_payload", [{"type": "stored", "data": b"abcdef", "len": 10}], BAD_SIZE, b"abcdefghij")
    add("stored_len_past_isize", [{"type": "stored", "data": b"abcdefghij"}], BAD_SIZE, b"abcdef")
    # a payload whose last token is a match with a 15-bit distance code and 13 extra bits: cut short, zlib runs out of input
    head = rng.integers(0, 256, 30000, dtype=np.uint8).tobytes()
    far = [{"type": "stored", "data": head}, dyn([97, (3, 24577 + 5000)], check=True, lit_lens=one["lit_lens"],
                                                 dist_lens=dw.assign(list(range(15)) + [29], dw.skewed_lengths(16, 15), 30))]
    text = dw.block_text(far)
    assert zlib.decompress(dw.write_stream(far), -15) == text
    for cut in range(1, 7):
        add("cut_%d_inside_a_15_bit_code_with_13_extra_bits" % cut, far, BAD_SIZE, text, cut=cut)
    valid = {n: (m, d) for n, m, d, _ in _foreign()}
    m, d = valid["everything_at_once"]
    add("everything_at_once/isize-1", payload_of(m), BAD_SIZE, d, isize=len(d) - 1)
    add("everything_at_once/crc", payload_of(m), BAD_CRC, d, crc=zlib.crc32(d) ^ 0x80000000)
    m, d = valid["size/33"]
    add("size/33/isize+1", payload_of(m), BAD_SIZE, d, isize=34)
    add("size/33/crc", payload_of(m), BAD_CRC, d, crc=zlib.crc32(d) ^ 1)
    # gzip members that are no BGZF members
    p = payload_of(m)
    for name, gz in (("fname", dict(flg=12, fname=b"rows.txt")), ("fhcrc", dict(flg=6, hcrc=True)), ("no_bc", dict(subfields=(("XY", b"\x01\x02"),))),
                     ("two_bc", dict(subfields=(("BC", None), ("BC", None)))), ("bc_of_4_bytes", dict(subfields=(("BC", b"\0\0\0\0"),)))):
        g = wrap_gzip(p, d, **gz)
        assert zlib.decompress(g, 31) == d and "wrapper/" + name in GZIP_NOT_BGZF
        out.append(("wrapper/" + name, g))
        FOREIGN_DAMAGED_EXPECT["wrapper/" + name] = BAD_HEADER
    _FOREIGN["damaged"] = out
    return out


def foreign_features(members):
    """the tracer over valid members [(name, member, data)]: its text must be zlib's; returns (Counter of the features of
    deflate_writer.trace summed over the members, plus what only a whole member shows; {name: the member's own Counter})"""
    import deflate_writer as dw
    total, per = Counter(), {}
    for name, m, data in members:
        xlen = struct.unpack_from("<H", m, 10)[0]
        payload = m[12 + xlen:-8]
        tr = dw.trace(payload)
        assert tr.text == zlib.decompress(payload, -15) == data, name
        f = tr.features
        kinds = [b[0] for b in tr.blocks]
        if len(kinds) >= 1000 and all(kinds[k] == (0, 1, 2)[k % 3] for k in range(len(kinds))):
            f["member_1000_blocks_cycling"] += 1
        if len(data) == 65536 and f["hlit:286"] and f["hdist:30"] and f["lit_bits:15"] and f["dist_bits:15"] and f["dist_32768"] and \
                all(f["len_sym:%d:min" % s] for s in range(257, 286)) and all(f["dist_sym:%d:max" % s] for s in range(30)):
            f["everything_at_once"] += 1
        subfields, at = [], 12
        while at < 12 + xlen:
            subfields.append(m[at:at + 2])
            at += 4 + struct.unpack_from("<H", m, at + 2)[0]
        if subfields.index(b"BC") > 0:
            f["wrapper_extra_before_bc"] += 1
        if subfields.index(b"BC") < len(subfields) - 1:
            f["wrapper_extra_behind_bc"] += 1
        if 0 < subfields.index(b"BC") < len(subfields) - 1:
            f["wrapper_extra_on_both_sides"] += 1
        if xlen > 6:
            f["wrapper_xlen_above_6"] += 1
        if m[4:8] != b"\0\0\0\0" and m[8] and m[9] != 255:
            f["wrapper_mtime_xfl_os"] += 1
        per[name] = f
        total.update(f)
    return total, per


def required_features():
    req = ["lit_bits:%d" % l for l in range(1, 16)] + ["dist_bits:%d" % l for l in range(1, 16)]
    req += ["len_sym:%d:%s" % (s, e) for s in range(257, 286) for e in ("min", "max")] + ["dist_sym:%d:%s" % (s, e) for s in range(30) for e in ("min", "max")]
    req += ["len258_as_285", "len258_as_284", "dist_32768", "dist_32507_32767", "dist_eq_written:32768", "dist_eq_written:1", "match_ends_at_65536_of_65536"]
    req += ["overlap:%d" % d for d in (1, 2, 3, 7, 63, 64, 65)] + ["overlap_257_len258", "src_ends_on_prev_literal"]
    # (HCLEN 4 cannot occur in a valid block -- see _foreign() -- so the smallest that can, 5, stands for it here)
    req += ["hlit:257", "hlit:286", "hdist:1", "hdist:30", "hclen:5", "hclen:19", "hclen19_slot18_nonzero", "cl_len7", "cl_bits:7"]
    req += ["rep16:3", "rep16:6", "rep17:3", "rep17:10", "rep18:11", "rep18:138", "rep16_cross", "rep17_cross", "rep18_cross"]
    req += ["dist_one_code_used", "lit_only_end_code", "hdist1_len0_no_match"]
    req += ["stored_len0_first", "stored_len0_middle", "stored_len0_final", "stored_len:65505", "stored_after_huffman_pad:0"]
    req += ["stored_after_huffman_pad:%d_ones" % k for k in range(1, 8)] + ["after_stored_pos_mod4:%d" % r for r in range(4)]
    req += ["member_1000_blocks_cycling", "dyn15_then_dyn2", "dyn2_then_dyn15", "fixed_after_dynamic", "final_ends_inside_byte_rest_ones", "trailing_bytes"]
    req += ["text_size:%d" % n for n in FOREIGN_SIZES] + ["everything_at_once"]
    req += ["wrapper_extra_before_bc", "wrapper_extra_behind_bc", "wrapper_extra_on_both_sides", "wrapper_xlen_above_6", "wrapper_mtime_xfl_os"]
    return req


# what the issue's table found absent from valid_corpus() (zlib's compressor does not write it)
ABSENT_FROM_ZLIB = ["dist_32768", "dist_32507_32767", "lit_bits:15", "len258_as_284", "hclen19_slot18_nonzero", "rep16_cross", "rep17_cross", "rep18_cross",
                    "dist_one_code_used"] + ["dist_bits:%d" % l for l in range(12, 16)]


def assert_features_hit(counter):
    missing = [k for k in required_features() if not counter[k]]
    assert not missing, "the foreign corpus misses: %s" % missing
