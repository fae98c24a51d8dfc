"""A small BAI writer for the test corpora (SAM/BAM specification 5.2 and 5.3: the binning index and reg2bin), independent of
basevar_amd/host/bamio.hpp, which reads what this writes.  A bin's chunks are the maximal series of consecutive records of that
bin; a virtual offset that falls on the end of a BGZF member is written as the start of the next one (a zero low half), which
is one of the two forms a writer may choose and the one a reader of whole members has to get right."""
import struct

import bam_py

REF_CONSUMING = {0, 2, 3, 7, 8}  # M D N = X


def reg2bin(beg, end):
    """the bin of [beg, end) (0-based): the smallest that holds it whole"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def index_records(bam_path):
    """-> (n_ref, [(tid, pos, end, flag, virtual offset, virtual offset behind it)]) of every record, in file order"""
    blocks = bam_py.bgzf_blocks(bam_path)
    data = b"".join(p for _, _, p in blocks)
    starts, at = [], 0
    for _, _, p in blocks:
        starts.append(at)
        at += len(p)

    def voff(o):
        for k, (off, _, p) in enumerate(blocks):
            if o < starts[k] + len(p):
                return (off << 16) | (o - starts[k])
        return blocks[-1][0] << 16  # the end of the stream: the end-of-file member

    assert data[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, o)
        o += 4 + l_name + 4
    out = []
    while o < len(data):
        bs, = struct.unpack_from("<i", data, o)
        tid, pos, l_rn, _mq, _bin, n_cig, flag, _l_seq = struct.unpack_from("<iiBBHHHi", data, o + 4)
        cig = struct.unpack_from("<%dI" % n_cig, data, o + 4 + 32 + l_rn)
        rlen = sum(c >> 4 for c in cig if (c & 15) in REF_CONSUMING)
        out.append((tid, pos, pos + (rlen or 1), flag, voff(o), voff(o + 4 + bs)))
        o += 4 + bs
    return n_ref, out


def write_bai(bam_path, bai_path=None):
    """<bam_path>.bai for a coordinate-sorted BAM file; returns {tid: {bin: [(beg, end)]}}"""
    n_ref, recs = index_records(bam_path)
    bins = [dict() for _ in range(n_ref)]
    linear = [dict() for _ in range(n_ref)]
    last = (None, None)
    for tid, pos, end, flag, vb, ve in recs:
        if tid < 0:
            last = (None, None)
            continue
        b = reg2bin(pos, end)
        chunks = bins[tid].setdefault(b, [])
        if last == (tid, b):
            chunks[-1] = (chunks[-1][0], ve)
        else:
            chunks.append((vb, ve))
        last = (tid, b)
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            linear[tid][w] = min(linear[tid].get(w, vb), vb)
    out = bytearray(b"BAI\x01" + struct.pack("<i", n_ref))
    for tid in range(n_ref):
        out += struct.pack("<i", len(bins[tid]))
        for b in sorted(bins[tid]):
            out += struct.pack("<Ii", b, len(bins[tid][b])) + b"".join(struct.pack("<QQ", *c) for c in bins[tid][b])
        n_intv = max(linear[tid]) + 1 if linear[tid] else 0
        offs, prev = [], 0
        for w in range(n_intv):
            prev = linear[tid].get(w, prev)
            offs.append(prev)
        out += struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *offs)
    with open(bai_path or bam_path + ".bai", "wb") as f:
        f.write(bytes(out))
    return {tid: bins[tid] for tid in range(n_ref)}
