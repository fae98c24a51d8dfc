"""The blocks and count vectors that the small level of the device DEFLATE encoder (basevar_amd/csrc/bv_deflate_small_core.h) is
held to beyond tests/deflate_corpus.py's: blocks built for what dynamic codes and three gram tables add -- the choice between
the three forms and its ties, the block header's fields and run symbols, which table a match comes from -- and count vectors
for the depth limit of the code-length construction.  tests/deflate_small_model.py says what every block becomes;
small_edge_report() says, from the tracer's reading of the members and from the model's account of its parse, where they went."""
import itertools

import numpy as np

import deflate_corpus as dc
import deflate_small_model as sm

MAX_BLOCK = dc.MAX_BLOCK


def de_bruijn(k, n):
    """the de Bruijn sequence B(k, n) as a list of 0 .. k - 1: every n-gram occurs once in the cyclic sequence"""
    a = [0] * (k * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


def no_repeat(letters, length=None):
    """text over `letters` in which no four bytes occur twice"""
    seq = de_bruijn(len(letters), 4)
    seq = (seq + seq[:3])[:length or len(seq) + 3]
    return bytes(letters[s] for s in seq)


def collision8():
    """two unequal 8-grams of upper-case letters, no byte in common, with one hash_8 and different hash_4"""
    rng = np.random.default_rng(31)
    first = {}
    for _ in range(3000):
        g = bytes(rng.choice(np.frombuffer(b"BCDEFGHI", np.uint8), 8))
        first.setdefault(sm.hash_g(g, 0, 8), g)
    for _ in range(3000):
        g = bytes(rng.choice(np.frombuffer(b"JKLMNOPQ", np.uint8), 8))
        other = first.get(sm.hash_g(g, 0, 8))
        if other is not None and sm.hash_g(other, 0, 4) != sm.hash_g(g, 0, 4):
            return other, g
    raise AssertionError("no collision found")


def _ties(pool):
    """from prefixes of the pool's texts: a block whose dynamic and fixed forms have the same bytes, fewer than stored (fixed is
    written), and blocks whose smallest coded form has exactly the stored form's bytes (stored is written)"""
    found = {}
    for text in pool:
        for n in range(1, min(len(text), 400)):
            info = {}
            sm.payload(text[:n], info)
            d, f, s = info["sizes"]
            if d == f < s:
                found.setdefault("dynamic_fixed", text[:n])
            if min(d, f) == s:
                found.setdefault("stored", text[:n])
            if d == s < f:
                found.setdefault("dynamic_stored", text[:n])
        if len(found) == 3:
            break
    return found


def small_edge_corpus(emit_exe):
    """[(name, [blocks])], every block 1 .. 0xff00 bytes"""
    rng = np.random.default_rng(29)
    out = []
    small = dc.emitted(emit_exe, "vcf", 1000, 3, 7)
    low = no_repeat(b"acgtnx")  # 1299 bytes below 128, skewed by nothing: dynamic codes of 2 and 3 bits

    # the three forms: VCF text (dynamic), a few bytes (fixed), random bytes (stored)
    out.append(("forms", [small[:3000], b"abc", b"ab" * 9, dc._rand(rng, 500)]))

    # ties between the forms, found among the prefixes of three kinds of text
    letters = np.frombuffer(b"eeeeeeeettttaaoinshr", np.uint8)[rng.integers(0, 20, 400)].tobytes()
    skew = np.frombuffer(bytes(range(150, 170)) + bytes([200]) * 20, np.uint8)[rng.integers(0, 40, 400)].tobytes()
    ties = _ties([small, letters, skew, low])
    out.append(("ties", [ties[k] for k in sorted(ties)]))

    # no match at all, in a block that dynamic codes win: the distance lengths are [1, 1]
    out.append(("no_match", [low, low[:700]]))

    # one distance symbol: runs of a byte that occurs nowhere else, inside text without repeats: every match lies 1 back
    body = bytearray()
    for k in range(24):
        body += low[50 * k:50 * k + 50] + bytes([0x80 + k]) * (12 + k)
    out.append(("one_distance", [bytes(body)]))

    # the header's run symbols.  Only bytes below 100 and no match: 156 zeros before the end code, 138 of them in one
    # symbol 18; bytes 0 and 255 only: 254 zeros; all 256 bytes at equal counts and matches: runs of equal non-zero lengths
    out.append(("runs", [no_repeat(b"\x01\x02\x03\x04\x05\x06\x07"), no_repeat(b"\x00\xff\x00\xff\x01"[:2] + b"\x20\x21\x22", 500),
                         bytes(range(256)) * 6 + bytes(range(255, -1, -1)) * 2, small[:20000]]))

    # a run of equal lengths from the literal into the distance lengths: periods of 1 .. 4 fresh bytes, each a match of 258
    # and one of 240, so that symbols 284 and 285 and distance symbols 0 .. 3 all get two bits
    blocks = []
    for rounds in (3, 5, 6):
        t, b = bytearray(), 255
        for _ in range(rounds):
            for d in (1, 2, 3, 4):
                t += (bytes(range(b - d + 1, b + 1)) * (600 // d))[:d + 258 + 240]
                b -= d
        blocks.append(bytes(t))
    out.append(("crossing", blocks))

    # which table gives the match
    a16 = b"0123456789:;<=>?"
    g1, g2 = collision8()
    blocks = [
        low[:100] + a16 + low[100:200] + a16 + b"!",                        # the 16-gram table
        low[:100] + a16[:11] + low[100:200] + a16[:11] + b"!",              # the 8-gram table: 11 bytes
        low[:100] + a16[:6] + low[100:200] + a16[:6] + b"!",                # the 4-gram table: 6 bytes
        # a 16-gram whose candidate lies beyond the window, its first 8 bytes within it
        a16 + b"a" * 32760 + a16[:8] + b"##" + a16 + b"!",
        # two 8-grams with one hash: the second takes the first's entry, the first's repeat comes from the 4-gram table
        low[:60] + g1 + low[60:120] + g2 + low[120:180] + g1 + b"!",
        low[:60] + g1 + low[60:120] + b"RSTUVWXY" + low[120:180] + g1 + b"!",  # (without the collision: the 8-gram table)
    ]
    out.append(("tables", blocks))

    # sizes 1 .. 300 of text that dynamic codes win from about 100 bytes on, and the two largest
    big = dc.emitted(emit_exe, "vcf", 10000, 3, 5)
    assert len(big) >= 2 * MAX_BLOCK - 1
    out.append(("sizes", [small[7 * n:8 * n] for n in range(1, 301)] + [big[:MAX_BLOCK - 1], big[MAX_BLOCK - 1:2 * MAX_BLOCK - 1]]))
    for name, blocks in out:
        assert all(1 <= len(b) <= MAX_BLOCK for b in blocks), name
    return out


def small_edge_report(members, blocks):
    """what the tracer (tests/deflate_writer.py) finds in the members, and what the model says about the parse of their blocks"""
    from collections import Counter
    rep = dict(forms=Counter(), features=Counter(), hclen=set(), taken=Counter(), refused=Counter(), no_match_dynamic=0, one_distance_dynamic=0)
    for m, block in zip(members, blocks):
        tr = dc.traced(m)
        assert tr.text == block and len(tr.blocks) == 1
        form = tr.blocks[0][0]
        rep["forms"][form] += 1
        matches = [t for t in tr.tokens if not isinstance(t, int)]
        if form == 2:
            f = tr.features
            rep["features"].update(k for k in f if k.startswith("rep"))
            rep["hclen"] |= {int(k.split(":")[1]) for k in f if k.startswith("hclen:")}
            if not matches and f["hdist:2"] == 1:
                rep["no_match_dynamic"] += 1
            # every match with the same distance symbol, and that symbol coded in one bit
            if matches and f["dist_bits:1"] == len(matches) and len({sm.distance_symbol(t[1])[0] for t in matches}) == 1:
                rep["one_distance_dynamic"] += 1
        if form != 0:
            taken = []
            assert sm.tokens(block, taken) == tr.tokens
            for g, refused, _ in taken:
                rep["taken"][g] += 1
                for r in refused:
                    rep["refused"][r + (g,)] += 1
    return rep


def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


# the rounds of halving that the named Fibonacci vectors need (16 and 8 of them fit their limit as they are)
FIBONACCI_ROUNDS = {"fibonacci_16_of_286": 0, "fibonacci_17_of_286": 1, "fibonacci_17_doubled_of_286": 2,
                    "fibonacci_16_of_30": 0, "fibonacci_17_of_30": 1, "fibonacci_17_doubled_of_30": 2,
                    "fibonacci_8_of_19": 0, "fibonacci_9_of_19": 1, "fibonacci_9_doubled_of_19": 2, "fibonacci_15_of_19": 2}


def count_vectors():
    """[(name, limit, counts)] for the code-length construction.  Fibonacci counts give the deepest tree a sum of counts can: k
    of them reach k - 1 bits, so 17 or more need a round of halving at limit 15, 9 or more at limit 7; how many rounds a vector
    takes is the model's to say.  Halving turns Fibonacci counts into shallower ones at once, so the vectors that need two rounds
    are Fibonacci counts doubled: one round gives the plain ones back.  FIBONACCI_ROUNDS names the vectors of one and of two
    rounds for every alphabet; the tests assert them."""
    out = []
    for nsym in (286, 30):
        for k in (16, 17, 18, 22):
            c = [0] * nsym
            for j, v in enumerate(fibonacci(k)):
                c[(j * 7 + 3) % nsym] = v  # (not in the order of the symbols)
            out.append(("fibonacci_%d_of_%d" % (k, nsym), 15, c))
        out.append(("fibonacci_17_doubled_of_%d" % nsym, 15, [2 * v for v in out[-3][2]]))
    for k in range(8, 20):
        out.append(("fibonacci_%d_of_19" % k, 7, (fibonacci(k)[::-1] + [0] * 19)[:19]))
    out.append(("fibonacci_9_doubled_of_19", 7, [2 * v for v in (fibonacci(9)[::-1] + [0] * 19)[:19]]))
    # powers of two: a chain as deep, which halving shortens by one leaf a round
    for nsym, limit, ks in ((286, 15, (16, 17, 18, 19, 20)), (30, 15, (16, 17, 18, 19, 20)), (19, 7, (8, 9, 10, 11, 12))):
        for k in ks:
            c = [0] * nsym
            for j in range(k):
                c[(j * 7 + 1) % nsym] = 1 << j
            out.append(("powers_%d_of_%d" % (k, nsym), limit, c))
    out.append(("fibonacci_286", 15, [min(v, 1 << 20) for v in fibonacci(286)]))
    for nsym, limit in ((286, 15), (30, 15), (19, 7)):
        out.append(("ones_%d" % nsym, limit, [1] * nsym))
        out.append(("one_symbol_%d" % nsym, limit, [0] * (nsym - 1) + [5]))
        out.append(("first_symbol_%d" % nsym, limit, [5] + [0] * (nsym - 1)))
        out.append(("no_symbol_%d" % nsym, limit, [0] * nsym))
        out.append(("equal_%d" % nsym, limit, [7] * (nsym - 3) + [0, 7, 7]))
        out.append(("two_values_%d" % nsym, limit, [3 if s % 3 else 2 for s in range(nsym)]))
    out.append(("one_count_of_65281", 15, [0] * 97 + [65281] + [0] * 188))
    out.append(("65281_and_the_end_code", 15, [0] * 97 + [65280] + [0] * 158 + [1] + [0] * 29))
    return out


def kraft_is_one(lengths):
    return sum(1 << (15 - l) for l in lengths if l) == 1 << 15


def format_vectors(vectors):
    """the count vectors as tests/cpp/deflate_core_check.cpp --lengths reads them"""
    return "".join("%d %d %s\n" % (limit, len(c), " ".join(str(x) for x in c)) for _, limit, c in vectors)
