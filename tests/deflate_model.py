"""What the device DEFLATE encoder writes, restated from the definition at the head of basevar_amd/csrc/bv_deflate_core.h and
from RFC 1951 / the SAM specification, not from the encoder's code: no chunks, no lanes, no `last` flags.

  cand(p)  the latest q < p whose four bytes hash as text[p .. p+4) does (both with four bytes inside the block)
  a match  at p: the common prefix of text[p ..) and text[cand(p) ..), at most min(258, n - p), if it is >= 4 and
           p - cand(p) <= 32768
  parse    greedy from p = 0: a match is taken whole, else text[p] is a literal
  stream   one final block with the fixed Huffman codes, or one stored block where the fixed form is not smaller
  member   18 bytes of BGZF header with BSIZE, the stream, CRC32, ISIZE

tokens() is the serial coder the header names: a head-of-chain table (hash -> latest position) into which every position goes.
tests/test_deflate_cpu.py holds the CPU build of the encoder to member(), byte for byte, tests/test_gpu_bgzf_deflate.py the
device; tests/deflate_writer.py's tracer (which shares nothing with this file but the tables of RFC 1951 3.2.5) and zlib read
what both write."""
import os
import re
import struct
import zlib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "basevar_amd", "csrc", "bv_deflate_core.h")
MIN_MATCH, MAX_MATCH, WINDOW, MAX_BLOCK = 4, 258, 32768, 0xff00

# RFC 1951 3.2.5: the first length / distance of every code and its extra bits
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def hash_bits():
    """BV_DEF_HASH_BITS as the header defines it"""
    with open(HEADER) as fh:
        found = re.findall(r"^\s*#\s*define\s+BV_DEF_HASH_BITS\s+(\d+)u?\s*$", fh.read(), re.M)
    assert len(found) == 1, found
    return int(found[0])


HASH_BITS = hash_bits()


def hash4(text, p):
    """the hash of the four bytes at p"""
    return ((int.from_bytes(text[p:p + 4], "little") * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def tokens(text):
    """the parse: an int is a literal byte, (length, distance) a match"""
    text = bytes(text)
    n = len(text)
    head = {}
    out = []
    cur = 0
    for p in range(n):
        cand = None
        if p + MIN_MATCH <= n:
            h = hash4(text, p)
            cand = head.get(h)
            head[h] = p
        if p < cur:  # inside a match that was taken: in the table, not coded
            continue
        length = 0
        if cand is not None and p - cand <= WINDOW:
            most = min(MAX_MATCH, n - p)
            if text[p:p + most] == text[cand:cand + most]:
                length = most
            else:
                while text[p + length] == text[cand + length]:
                    length += 1
        if length >= MIN_MATCH:
            out.append((length, p - cand))
            cur = p + length
        else:
            out.append(text[p])
            cur = p + 1
    return out


class _Bits:
    """RFC 1951 3.1.1: values go in from the low bit of a byte up, Huffman codes with their first bit first"""

    def __init__(self):
        self.done, self.acc, self.n = bytearray(), 0, 0

    def value(self, v, nbits):
        self.acc |= v << self.n
        self.n += nbits
        while self.n >= 8:
            self.done.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        self.value(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def bits(self):
        return 8 * len(self.done) + self.n

    def bytes(self):
        return bytes(self.done) + (bytes([self.acc]) if self.n else b"")


def _lit_len_code(sym):
    """RFC 1951 3.2.6: the fixed code of literal/length symbol sym"""
    if sym < 144:
        return 0b00110000 + sym, 8
    if sym < 256:
        return 0b110010000 + (sym - 144), 9
    if sym < 280:
        return sym - 256, 7
    return 0b11000000 + (sym - 280), 8


def _fixed(toks):
    b = _Bits()
    b.value(1, 1)
    b.value(1, 2)
    for t in toks:
        if isinstance(t, int):
            b.code(*_lit_len_code(t))
            continue
        length, dist = t
        assert MIN_MATCH <= length <= MAX_MATCH and 1 <= dist <= WINDOW, t
        s = max(k for k in range(29) if LEN_BASE[k] <= length)
        b.code(*_lit_len_code(257 + s))
        b.value(length - LEN_BASE[s], LEN_EXTRA[s])
        s = max(k for k in range(30) if DIST_BASE[k] <= dist)
        b.code(s, 5)
        b.value(dist - DIST_BASE[s], DIST_EXTRA[s])
    b.code(*_lit_len_code(256))
    return b


def fixed_payload(toks):
    """the tokens as one final block with the fixed codes; the bits behind the end code in the last byte are zero"""
    return _fixed(toks).bytes()


def fixed_bits(toks):
    """the bits of that block, from BFINAL to the end code"""
    return _fixed(toks).bits()


def stored_payload(text):
    n = len(text)
    return bytes([1]) + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(text)


def payload(text):
    """The raw DEFLATE stream of a block: the fixed form if it is smaller than the stored form's 5 + n bytes, else the stored.

    That comparison of the two finished sizes is all there is to the encoder's choice, although bv_def_put stops storing
    early (`over`): it does so only when four more whole bytes are due behind 2 + (5 + n) bytes counted from out + 16, so the
    finished fixed payload would have more than 5 + n bytes and loses the comparison anyway; and a stream that never
    trips it is compared as here."""
    assert 1 <= len(text) <= MAX_BLOCK
    fixed = fixed_payload(tokens(text))
    return fixed if len(fixed) < 5 + len(text) else stored_payload(text)


def member(text):
    """the whole BGZF member (SAM specification 4.1) of a block"""
    text = bytes(text)
    p = payload(text)
    total = 18 + len(p) + 8
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0]) + b"BC" + struct.pack("<HH", 2, total - 1) + p +
            struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text)))
