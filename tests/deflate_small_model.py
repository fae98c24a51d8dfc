"""What the device DEFLATE encoder writes at its small level (BV_DEFLATE_SMALL), restated from the definition at the head of
basevar_amd/csrc/bv_deflate_small_core.h and from RFC 1951, not from the encoder's code: no chunks, no lanes, no windows of
bits.  It shares with tests/deflate_model.py the tables of RFC 1951 3.2.5, the bit writer, the fixed code and the stored form.

  parse    three head-of-chain tables, for the 4-, 8- and 16-byte gram at every position; the match at p is the first of
           16, 8, 4 whose candidate exists, lies within 32768 and agrees with p for at least the gram's bytes; greedy
  lengths  Huffman by two queues over the symbols sorted by (count, symbol), leaf before internal node on a tie; counts halved
           (rounding up) and the tree rebuilt while it is deeper than the limit
  header   HLIT / HDIST / HCLEN as small as the lengths allow, the lengths spelled greedily with 16, 17 and 18
  choice   dynamic if smaller than fixed and than stored; else fixed if smaller than stored; else stored"""
import struct
import zlib

import numpy as np

import deflate_model as dm

K = 2654435761
HASH_BITS = 12
GRAMS = (16, 8, 4)
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def hash_g(text, p, g):
    v = 0
    for k in range(0, g, 4):
        v = (v * K + int.from_bytes(text[p + k:p + k + 4], "little")) & 0xFFFFFFFF
    return ((v * K) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def hashes(text, g):
    """hash_g at every position with g bytes inside the text (the same arithmetic, all positions at once)"""
    n = len(text)
    if n < g:
        return []
    b = np.frombuffer(text, np.uint8).astype(np.uint64)
    v = np.zeros(n - g + 1, np.uint64)
    for k in range(0, g, 4):
        w = sum(b[k + j:n - g + 1 + k + j] << np.uint64(8 * j) for j in range(4))
        v = (v * np.uint64(K) + w) & np.uint64(0xFFFFFFFF)
    return (((v * np.uint64(K)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)).tolist()


def common_prefix(text, p, q, most):
    if text[p:p + most] == text[q:q + most]:
        return most
    k = 0
    while text[p + k] == text[q + k]:
        k += 1
    return k


def tokens(text, taken=None):
    """the parse: an int is a literal byte, (length, distance) a match.  taken: a list that receives, per match, the gram
    whose table gave it and the grams whose candidates were refused before it"""
    text = bytes(text)
    n = len(text)
    heads = {g: {} for g in GRAMS}
    hashed = {g: hashes(text, g) for g in GRAMS}
    out = []
    cur = 0
    for p in range(n):
        cand = {}
        for g in GRAMS:
            if p + g <= n:
                h = hashed[g][p]
                cand[g] = heads[g].get(h)
                heads[g][h] = p
        if p < cur:
            continue
        most = min(dm.MAX_MATCH, n - p)
        match, refused = None, []
        for g in GRAMS:
            q = cand.get(g)
            if q is None:
                continue
            if p - q > dm.WINDOW:
                refused.append((g, "window"))
                continue
            length = common_prefix(text, p, q, most)
            if length >= g:
                match = (length, p - q)
                if taken is not None:
                    taken.append((g, tuple(refused), text[q:q + g] != text[p:p + g]))
                break
            refused.append((g, "collision" if text[q:q + g] != text[p:p + g] else "short"))
        if match:
            out.append(match)
            cur = p + match[0]
        else:
            out.append(text[p])
            cur = p + 1
    return out


def length_symbol(length):
    s = max(k for k in range(29) if dm.LEN_BASE[k] <= length)
    return 257 + s, dm.LEN_EXTRA[s], length - dm.LEN_BASE[s]


def distance_symbol(dist):
    s = max(k for k in range(30) if dm.DIST_BASE[k] <= dist)
    return s, dm.DIST_EXTRA[s], dist - dm.DIST_BASE[s]


def counts(toks):
    ll, dd = [0] * 286, [0] * 30
    for t in toks:
        if isinstance(t, int):
            ll[t] += 1
        else:
            ll[length_symbol(t[0])[0]] += 1
            dd[distance_symbol(t[1])[0]] += 1
    ll[256] += 1
    return ll, dd


def code_lengths(cnt, limit):
    """(lengths, rounds) of the counts of one alphabet"""
    c = list(cnt)
    assert 2 <= len(c) <= 1 << limit
    while sum(1 for x in c if x) < 2:
        c[c.index(0)] = 1
    rounds = 0
    while True:
        leaves = sorted((x, s) for s, x in enumerate(c) if x)
        # nodes: (weight, [symbols below]); two queues
        q1 = [(w, [s]) for w, s in leaves]
        q2 = []
        depth = {s: 0 for _, s in leaves}
        i1 = i2 = 0
        while (len(q1) - i1) + (len(q2) - i2) > 1:
            picked = []
            for _ in range(2):
                if i1 < len(q1) and (i2 >= len(q2) or q1[i1][0] <= q2[i2][0]):
                    picked.append(q1[i1])
                    i1 += 1
                else:
                    picked.append(q2[i2])
                    i2 += 1
            syms = picked[0][1] + picked[1][1]
            for s in syms:
                depth[s] += 1
            q2.append((picked[0][0] + picked[1][0], syms))
        if max(depth.values()) <= limit:
            break
        c = [(x + 1) // 2 if x else 0 for x in c]
        rounds += 1
    return [depth.get(s, 0) for s in range(len(c))], rounds


def canonical(lengths):
    """RFC 1951 3.2.2: {symbol: (code, bits)}"""
    bl = [0] * 17
    for l in lengths:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def spell(seq):
    """the code-length symbols of the joined lengths: [(symbol, extra value, extra bits)]"""
    out, i = [], 0
    while i < len(seq):
        v = seq[i]
        r = 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            if r <= 10:
                out.append((17, r - 3, 3))
                i += r
            else:
                t = min(r, 138)
                out.append((18, t - 11, 7))
                i += t
        elif v != 0 and i > 0 and seq[i - 1] == v and r >= 3:
            t = min(r, 6)
            out.append((16, t - 3, 2))
            i += t
        else:
            out.append((v, 0, 0))
            i += 1
    return out


def header(ll_len, d_len):
    """dict(hlit, hdist, hclen, spelled, cl_len) of a dynamic block with these lengths"""
    hlit = max(257, 1 + max(s for s in range(286) if ll_len[s]))
    hdist = max(1, 1 + max(s for s in range(30) if d_len[s]))
    spelled = spell(ll_len[:hlit] + d_len[:hdist])
    cl_cnt = [0] * 19
    for s, _, _ in spelled:
        cl_cnt[s] += 1
    cl_len, cl_rounds = code_lengths(cl_cnt, 7)
    hclen = max(4, 1 + max(k for k in range(19) if cl_len[CL_ORDER[k]]))
    return dict(hlit=hlit, hdist=hdist, hclen=hclen, spelled=spelled, cl_len=cl_len, cl_rounds=cl_rounds)


def _body(b, toks, ll, dd):
    for t in toks + [256]:
        if isinstance(t, int):
            b.code(*ll[t])
            continue
        s, eb, ev = length_symbol(t[0])
        b.code(*ll[s])
        b.value(ev, eb)
        s, eb, ev = distance_symbol(t[1])
        b.code(*dd[s])
        b.value(ev, eb)


def dynamic_payload(toks, info=None):
    ll_cnt, d_cnt = counts(toks)
    ll_len, ll_rounds = code_lengths(ll_cnt, 15)
    d_len, d_rounds = code_lengths(d_cnt, 15)
    h = header(ll_len, d_len)
    if info is not None:
        info.update(h, ll_len=ll_len, d_len=d_len, rounds=(ll_rounds, d_rounds, h["cl_rounds"]))
    b = dm._Bits()
    b.value(1, 1)
    b.value(2, 2)
    b.value(h["hlit"] - 257, 5)
    b.value(h["hdist"] - 1, 5)
    b.value(h["hclen"] - 4, 4)
    for k in range(h["hclen"]):
        b.value(h["cl_len"][CL_ORDER[k]], 3)
    cl = canonical(h["cl_len"])
    for s, ev, eb in h["spelled"]:
        b.code(*cl[s])
        b.value(ev, eb)
    _body(b, toks, canonical(ll_len), canonical(d_len))
    return b.bytes()


def payload(text, info=None):
    assert 1 <= len(text) <= dm.MAX_BLOCK
    toks = tokens(text)
    dyn = dynamic_payload(toks, info)
    fixed = dm.fixed_payload(toks)
    stored = 5 + len(text)
    if info is not None:
        info.update(sizes=(len(dyn), len(fixed), stored))
    if len(dyn) < len(fixed) and len(dyn) < stored:
        return dyn
    if len(fixed) < stored:
        return fixed
    return dm.stored_payload(text)


def member(text, info=None):
    """the whole BGZF member of a block at the small level"""
    text = bytes(text)
    p = payload(text, info)
    total = 18 + len(p) + 8
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0]) + b"BC" + struct.pack("<HH", 2, total - 1) + p +
            struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text)))
