"""A DEFLATE (RFC 1951) writer that encodes what it is told, not what compresses best, and a tracer that says what a stream
holds.  tests/bgzf_corpus.py builds its foreign corpus with them: streams that zlib's inflate accepts and zlib's deflate never
writes (other compressors do).  zlib stays the judge of every stream; the tracer only names the features.

Tokens: an int is a literal byte; (length, distance) is a match, (length, distance, True) spells length 258 as symbol 284 with
extra bits 31; ("sym", s) writes literal/length symbol s and nothing else; ("bits", value, n) writes n raw bits (the last two
are for damaged streams).

Blocks (dicts):
  {"type": "stored", "data": bytes, "pad": 0 or 1 (the padding bits before LEN; 1: all ones), "len": LEN written if not len(data)}
  {"type": "fixed", "tokens": [...]}
  {"type": "dynamic", "tokens": [...],
   "lit_lens": lengths of symbols 0 .. (default: a balanced code over the symbols the tokens use and 256),
   "dist_lens": the same for distances (default: balanced over the distance symbols used; none used: one length of 0),
   "hlit": number of literal/length lengths sent, 257 .. 286 (default: up to the last non-zero one; larger pads with zeros),
   "hdist": 1 .. 30, likewise, "hclen": 4 .. 19 (default: up to the last slot in use),
   "cl_lens": {symbol of the code-length code: its length} (default: balanced over the symbols the spelling uses),
   "spell": "plain" (one length per item), "rle" (greedy 16/17/18, free to cross from literal into distance lengths) or a
            list of ops: an int is a plain length, ("r16", count), ("r17", count), ("r18", count),
   "check": False lets through what a valid stream cannot hold (over-subscribed or incomplete sets, repeats that do not
            spell the lengths, symbols without a code are still an error)}
Every block may carry "final": 0 or 1; by default only the last block is final."""
import functools
from collections import Counter

from bgzf_corpus import CL_ORDER, Bits, _canonical

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
REP_BITS = {16: (2, 3), 17: (3, 3), 18: (7, 11)}  # extra bits, smallest count


def length_symbol(length, alt258=False):
    """(symbol, extra bits, extra value) of a match length"""
    assert 3 <= length <= 258, length
    if length == 258:
        return (284, 5, 31) if alt258 else (285, 0, 0)
    assert not alt258
    s = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]


def distance_symbol(distance):
    assert 1 <= distance <= 32768, distance
    s = max(k for k in range(30) if DIST_BASE[k] <= distance)
    return s, DIST_EXTRA[s], distance - DIST_BASE[s]


def expand(tokens, check=True):
    """the text the tokens stand for"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t[0], str):
            assert not check, t
        else:
            length, dist = t[0], t[1]
            assert not check or 1 <= dist <= len(out), (t, len(out))
            if dist > len(out):
                break
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


def kraft(lens):
    """sum of 2 ** -length over the coded symbols, in units of 2 ** -15"""
    return sum(1 << (15 - l) for l in lens if l)


def balanced_lengths(n):
    """a complete code over n symbols whose lengths differ by at most one (n = 1: one code of one bit, which is incomplete)"""
    if n <= 2:
        return [1] * n
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


def skewed_lengths(n, max_len):
    """a complete code over n symbols, ascending: 1, 2, ..., max_len - 1, max_len, max_len, with the shortest code split into
    two of one bit more until there are n.  Every length from the shortest that is left up to max_len occurs; with
    n = max_len + 1 that is every length from 1 (no complete code with more symbols has one code of each length 1 .. max_len:
    their Kraft sum alone is 1 - 2 ** -max_len)."""
    return list(_skewed_lengths(n, max_len))


@functools.lru_cache(maxsize=None)
def _skewed_lengths(n, max_len):
    assert max_len + 1 <= n <= 1 << max_len, (n, max_len)
    lens = list(range(1, max_len)) + [max_len, max_len]
    while len(lens) < n:
        l = lens.pop(0)
        assert l < max_len
        lens += [l + 1, l + 1]
        lens.sort()
    assert kraft(lens) == 1 << 15 and lens[-1] == max_len
    return tuple(lens)


def assign(symbols, lengths, n):
    """code lengths of an alphabet of n symbols: symbols[k] gets lengths[k], every other symbol 0"""
    assert len(symbols) == len(lengths) == len(set(symbols))
    out = [0] * n
    for s, l in zip(symbols, lengths):
        out[s] = l
    return out


def _used(tokens):
    lit, dist = Counter({256: 1}), Counter()
    for t in tokens:
        if isinstance(t, int):
            lit[t] += 1
        elif t[0] == "sym":
            lit[t[1]] += 1
        elif t[0] != "bits":
            lit[length_symbol(t[0], len(t) > 2 and t[2])[0]] += 1
            dist[distance_symbol(t[1])[0]] += 1
    return lit, dist


def by_frequency(counter, lengths_for):
    """lengths for the used symbols, the shortest codes to the most frequent: lengths_for(n) gives n ascending lengths"""
    syms = [s for s, _ in sorted(counter.items(), key=lambda kv: (-kv[1], kv[0]))]
    return syms, lengths_for(len(syms))


def spell_lengths(seq, mode):
    """the ops that spell the code lengths seq: "plain", or "rle" with the longest repeats that fit"""
    if mode == "plain":
        return list(seq)
    ops, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            take = min(run, 138)
            ops.append(("r18" if take >= 11 else "r17", take))
            i += take
        elif v != 0 and run >= 4:
            take = min(run - 1, 6)
            ops += [v, ("r16", take)]
            i += 1 + take
        else:
            ops.append(v)
            i += 1
    return ops


def _unspell(ops):
    out = []
    for o in ops:
        if isinstance(o, int):
            out.append(o)
        else:
            out += [out[-1] if o[0] == "r16" and out else 0] * o[1]
    return out


def _write_tokens(b, tokens, lit_codes, dist_codes):
    for t in tokens:
        if isinstance(t, int):
            b.code(*lit_codes[t])
        elif t[0] == "bits":
            b.put(t[1], t[2])
        elif t[0] == "sym":
            b.code(*lit_codes[t[1]])
        else:
            s, eb, ev = length_symbol(t[0], len(t) > 2 and t[2])
            b.code(*lit_codes[s]).put(ev, eb)
            s, eb, ev = distance_symbol(t[1])
            b.code(*dist_codes[s]).put(ev, eb)
    if 256 in lit_codes:  # (a damaged block may have no end code)
        b.code(*lit_codes[256])


def _write_dynamic(b, blk):
    tokens, check = blk["tokens"], blk.get("check", True)
    lit_used, dist_used = _used(tokens)
    lit_lens = blk.get("lit_lens")
    if lit_lens is None:
        lit_lens = assign(*by_frequency(lit_used, balanced_lengths), 286)
    dist_lens = blk.get("dist_lens")
    if dist_lens is None:
        dist_lens = assign(*by_frequency(dist_used, balanced_lengths), 30) if dist_used else [0]
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    if check:
        for name, lens in (("literal/length", lit_lens), ("distance", dist_lens)):
            k = kraft(lens)
            assert k == 1 << 15 or (k == 1 << 14 and max(lens) == 1) or k == 0, "%s lengths: Kraft sum %d / 32768" % (name, k)
        assert lit_lens[256:257] and lit_lens[256]
    hlit = blk.get("hlit") or max(257, max(k + 1 for k, l in enumerate(lit_lens) if l) if any(lit_lens) else 257)
    hdist = blk.get("hdist") or max(1, max(k + 1 for k, l in enumerate(dist_lens) if l) if any(dist_lens) else 1)
    assert 257 <= hlit <= 286 and 1 <= hdist <= 30 and not any(lit_lens[hlit:]) and not any(dist_lens[hdist:])
    seq = (lit_lens + [0] * 286)[:hlit] + (dist_lens + [0] * 30)[:hdist]
    spell = blk.get("spell", "rle")
    ops = spell_lengths(seq, spell) if isinstance(spell, str) else list(spell)
    if check:
        assert _unspell(ops) == seq, "the ops do not spell the code lengths"
    items = []
    for o in ops:
        if isinstance(o, int):
            items.append((o, 0))
        else:
            sym = int(o[0][1:])
            assert 0 <= o[1] - REP_BITS[sym][1] < 1 << REP_BITS[sym][0], o
            items.append((sym, o[1] - REP_BITS[sym][1]))
    cl_lens = blk.get("cl_lens")
    if cl_lens is None:
        cl_used = Counter(s for s, _ in items)
        if len(cl_used) == 1:  # the code-length code may not be incomplete: a second code that nothing uses
            cl_used[0 if 0 not in cl_used else 8] += 0
        cl_lens = dict(zip(*by_frequency(cl_used, balanced_lengths)))
    if check:
        assert kraft(cl_lens.values()) == 1 << 15 and max(cl_lens.values()) <= 7, cl_lens
    last = max([CL_ORDER.index(s) for s, l in cl_lens.items() if l] + [3]) + 1
    hclen = blk.get("hclen") or last
    assert last <= hclen <= 19 or not check
    b.put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        b.put(cl_lens.get(s, 0), 3)
    cl_codes = _canonical([cl_lens.get(s, 0) for s in range(19)])
    for s, extra in items:
        b.code(*cl_codes[s])
        if s >= 16:
            b.put(extra, REP_BITS[s][0])
    _write_tokens(b, tokens, _canonical(lit_lens), _canonical(dist_lens))


def write_stream(blocks, trailing=b"", end_fill=1):
    """the blocks as one raw DEFLATE stream; the bits of the last byte behind the final block are end_fill; then `trailing`"""
    b = Bits()
    for k, blk in enumerate(blocks):
        b.put(blk.get("final", int(k == len(blocks) - 1)), 1)
        if blk["type"] == "stored":
            data = blk["data"]
            b.put(0, 2)
            pad = -b.n % 8
            b.put(((1 << pad) - 1) if blk.get("pad", 0) else 0, pad)
            n = blk.get("len", len(data))
            b.put(n, 16).put(blk.get("nlen", n ^ 0xFFFF), 16)
            b.put(int.from_bytes(data, "little"), 8 * len(data))
        elif blk["type"] == "fixed":
            b.put(1, 2)
            fixed = _canonical(FIXED_LIT_LENS)
            _write_tokens(b, blk["tokens"], fixed, {s: (s, 5) for s in range(30)})
        else:
            _write_dynamic(b, blk)
    pad = -b.n % 8
    b.put(((1 << pad) - 1) if end_fill else 0, pad)
    return b.bytes() + bytes(trailing)


assert _canonical(FIXED_LIT_LENS)[0] == (0x30, 8) and _canonical(FIXED_LIT_LENS)[256] == (0, 7)  # (the code of RFC 1951 3.2.6)


def block_text(blocks):
    """the text of a list of blocks (matches reach back across blocks)"""
    tokens = []
    for blk in blocks:
        tokens += list(blk["data"]) if blk["type"] == "stored" else [t for t in blk["tokens"]]
    return expand(tokens)


# ---------------------------------------------------------------------------------------------------------------------------
# the tracer


class TraceError(ValueError):
    pass


class Trace:
    def __init__(self, text, tokens, features, blocks):
        self.text, self.tokens, self.features, self.blocks = text, tokens, features, blocks


def _decode(bit, count, symbols):
    """one symbol of a canonical code, a bit at a time (zlib's contrib/puff): (symbol, bits taken)"""
    code = first = index = 0
    for l in range(1, 16):
        code |= bit()
        c = count[l]
        if code - c < first:
            return symbols[index + (code - first)], l
        index += c
        first = (first + c) << 1
        code <<= 1
    raise TraceError("no such code")


def _tables(lens):
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    symbols = [s for l in range(1, 16) for s, x in enumerate(lens) if x == l]
    left = 1
    for l in range(1, 16):
        left = left * 2 - count[l]
        if left < 0:
            raise TraceError("over-subscribed")
    return count, symbols, left


def trace(payload):
    """Decode a raw DEFLATE stream bit by bit: Trace(text, tokens, features, blocks).  tokens are this module's (a stored block
    gives its bytes as literals); blocks is [(type, first token, first text byte)]; features is a Counter of names:
      lit_bits:L, dist_bits:L, cl_bits:L   codes of L bits decoded      len_sym:S:min / :max, dist_sym:S:min / :max
      len258_as_285 / _as_284              dist_32768, dist_32507_32767  dist_eq_written, dist_eq_written:D
      overlap:D (distance < length)        overlap_257_len258            src_ends_on_prev_literal
      hlit:N hdist:N hclen:N               hclen19_slot18_nonzero        cl_len7
      rep16:C rep17:C rep18:C              rep16_cross rep17_cross rep18_cross (from literal into distance lengths)
      dist_one_code_used                   lit_only_end_code             hdist1_len0_no_match
      stored_len:N                         stored_len0_first / _middle / _final
      stored_after_huffman_pad:K           ..._pad:K_ones (K > 0 padding bits, all ones)
      after_stored_pos_mod4:R              (where the next block starts in the payload)
      blocks:T per block type              dyn15_then_dyn2, dyn2_then_dyn15, fixed_after_dynamic
      final_ends_inside_byte_rest_ones     trailing_bytes                text_size:N    match_ends_at_65536_of_65536"""
    data = bytes(payload)
    nbits = len(data) * 8
    pos = 0
    f = Counter()
    out = bytearray()
    tokens, blocks = [], []

    def bit():
        nonlocal pos
        if pos >= nbits:
            raise TraceError("out of input")
        v = (data[pos >> 3] >> (pos & 7)) & 1
        pos += 1
        return v

    def bits(n):
        v = 0
        for k in range(n):
            v |= bit() << k
        return v

    prev_kind, prev_max, final, last_match_end = None, 0, 0, -1
    while not final:
        final = bit()
        btype = bits(2)
        blocks.append((btype, len(tokens), len(out)))
        f["blocks:%d" % btype] += 1
        if btype == 3:
            raise TraceError("block type 3")
        if btype == 0:
            pad = -pos % 8
            padv = bits(pad)
            if prev_kind in (1, 2):
                f["stored_after_huffman_pad:%d" % pad] += 1
                if pad and padv == (1 << pad) - 1:
                    f["stored_after_huffman_pad:%d_ones" % pad] += 1
            n, nn = bits(16), bits(16)
            if n != nn ^ 0xFFFF:
                raise TraceError("LEN / NLEN")
            if pos + 8 * n > nbits:
                raise TraceError("out of input")
            chunk = data[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
            out += chunk
            tokens += list(chunk)
            f["stored_len:%d" % n] += 1
            if n == 0:
                f["stored_len0_" + ("final" if final else "first" if len(blocks) == 1 else "middle")] += 1
            if not final:
                f["after_stored_pos_mod4:%d" % ((pos >> 3) & 3)] += 1
            prev_kind, prev_max = 0, 0
            continue
        if btype == 1:
            lit_lens, dist_lens = FIXED_LIT_LENS, [5] * 32  # (symbols 286, 287, 30 and 31 have codes and no meaning)
            if prev_kind == 2:
                f["fixed_after_dynamic"] += 1
            this_max = 9
        else:
            nl, nd, nc = bits(5) + 257, bits(5) + 1, bits(4) + 4
            if nl > 286 or nd > 30:
                raise TraceError("HLIT / HDIST")
            f["hlit:%d" % nl] += 1
            f["hdist:%d" % nd] += 1
            f["hclen:%d" % nc] += 1
            cl = [0] * 19
            for k in range(nc):
                cl[CL_ORDER[k]] = bits(3)
            if nc == 19 and cl[15]:
                f["hclen19_slot18_nonzero"] += 1
            if 7 in cl:
                f["cl_len7"] += 1
            count, symbols, left = _tables(cl)
            if left:
                raise TraceError("code-length code incomplete")
            lens = []
            while len(lens) < nl + nd:
                s, l = _decode(bit, count, symbols)
                f["cl_bits:%d" % l] += 1
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16 and not lens:
                    raise TraceError("repeat without a previous length")
                rep = REP_BITS[s][1] + bits(REP_BITS[s][0])
                f["rep%d:%d" % (s, rep)] += 1
                if len(lens) < nl < len(lens) + rep:
                    f["rep%d_cross" % s] += 1
                lens += [lens[-1] if s == 16 else 0] * rep
            if len(lens) > nl + nd:
                raise TraceError("repeat past the end")
            lit_lens, dist_lens = lens[:nl], lens[nl:]
            if not lit_lens[256]:
                raise TraceError("no end-of-block code")
            this_max = max(lens)
            if prev_kind == 2 and prev_max == 15 and this_max <= 2:
                f["dyn15_then_dyn2"] += 1
            if prev_kind == 2 and prev_max <= 2 and this_max == 15:
                f["dyn2_then_dyn15"] += 1
        lcount, lsyms, lleft = _tables(lit_lens)
        dcount, dsyms, dleft = _tables(dist_lens)
        for left, lens in ((lleft, lit_lens), (dleft, dist_lens)):
            if left and max(lens) > 1:
                raise TraceError("incomplete set")
        matches = 0
        while True:
            s, l = _decode(bit, lcount, lsyms)
            f["lit_bits:%d" % l] += 1
            if s < 256:
                out.append(s)
                tokens.append(s)
                continue
            if s == 256:
                break
            if s > 285:
                raise TraceError("length symbol %d" % s)
            ev = bits(LEN_EXTRA[s - 257])
            alt = s == 284 and ev == 31
            length = LEN_BASE[s - 257] + ev
            if ev == 0:
                f["len_sym:%d:min" % s] += 1
            if ev == (1 << LEN_EXTRA[s - 257]) - 1:
                f["len_sym:%d:max" % s] += 1
            if length == 258:
                f["len258_as_284" if alt else "len258_as_285"] += 1
            d, l = _decode(bit, dcount, dsyms)
            f["dist_bits:%d" % l] += 1
            if d > 29:
                raise TraceError("distance symbol %d" % d)
            ev = bits(DIST_EXTRA[d])
            dist = DIST_BASE[d] + ev
            if ev == 0:
                f["dist_sym:%d:min" % d] += 1
            if ev == (1 << DIST_EXTRA[d]) - 1:
                f["dist_sym:%d:max" % d] += 1
            if dist > len(out):
                raise TraceError("distance %d with %d bytes written" % (dist, len(out)))
            if dist == 32768:
                f["dist_32768"] += 1
            if 32507 <= dist <= 32767:
                f["dist_32507_32767"] += 1
            if dist == len(out):
                f["dist_eq_written"] += 1
                f["dist_eq_written:%d" % dist] += 1
            if dist < length:
                f["overlap:%d" % dist] += 1
                if dist == 257 and length == 258:
                    f["overlap_257_len258"] += 1
            if dist == length and tokens and isinstance(tokens[-1], int) and blocks[-1][1] < len(tokens):
                f["src_ends_on_prev_literal"] += 1
            matches += 1
            tokens.append((length, dist, True) if alt else (length, dist))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
            last_match_end = len(out)
        if btype == 2:
            if sum(1 for x in dist_lens if x) == 1 and max(dist_lens) == 1 and matches:
                f["dist_one_code_used"] += 1
            if sum(1 for x in lit_lens if x) == 1:
                f["lit_only_end_code"] += 1
            if nd == 1 and dist_lens[0] == 0 and not matches:
                f["hdist1_len0_no_match"] += 1
        prev_kind, prev_max = btype, this_max
    if pos % 8:
        rest = 8 - pos % 8
        if bits(rest) == (1 << rest) - 1:
            f["final_ends_inside_byte_rest_ones"] += 1
    if pos < nbits:
        f["trailing_bytes"] += 1
    f["text_size:%d" % len(out)] += 1
    if len(out) == 65536 and last_match_end == 65536:
        f["match_ends_at_65536_of_65536"] += 1
    return Trace(bytes(out), tokens, f, blocks)


# ---------------------------------------------------------------------------------------------------------------------------


def transcode(payload, max_len=15, cut=300, stored_every=0, deep_every=2, lit_alphabet=286, dist_alphabet=30, extra_tokens=()):
    """The tokens of an existing stream (read with the tracer), then extra_tokens, written again: dynamic blocks of `cut` tokens
    each under skewed codes of up to max_len bits over the whole of both alphabets (the shortest codes to the block's most
    frequent symbols; in every deep_every-th block to the symbols it does not use, so that its data is in the longest codes),
    all lengths spelled plainly so that HCLEN is 19, and every stored_every-th block stored."""
    tokens = trace(payload).tokens + list(extra_tokens)
    text = expand(tokens)
    blocks, at = [], 0
    for k, lo in enumerate(range(0, max(len(tokens), 1), cut)):
        part = tokens[lo:lo + cut]
        n = sum(1 if isinstance(t, int) else t[0] for t in part)
        if stored_every and k % stored_every == stored_every - 1:
            blocks.append({"type": "stored", "data": text[at:at + n], "pad": 1})
        else:
            lit, dist = _used(part)
            lit_syms = [s for s, _ in sorted(lit.items(), key=lambda kv: (-kv[1], kv[0]))] + [s for s in range(lit_alphabet) if s not in lit]
            dist_syms = [s for s, _ in sorted(dist.items(), key=lambda kv: (-kv[1], kv[0]))] + [s for s in range(dist_alphabet) if s not in dist]
            if deep_every and k % deep_every == deep_every - 1:
                lit_syms, dist_syms = lit_syms[::-1], dist_syms[::-1]
            blocks.append({"type": "dynamic", "tokens": part, "lit_lens": assign(lit_syms, skewed_lengths(len(lit_syms), max_len), 286),
                           "dist_lens": assign(dist_syms, skewed_lengths(len(dist_syms), max_len), 30), "spell": "plain"})
        at += n
    return write_stream(blocks), text
