"""A serial model of the rows of a region (include/basevar_amd_region.h; the definition stands at the head of
basevar_amd/csrc/bv_text_region_core.h).  It shares no code with the core: lines come from bytes.find, heads from a regular
expression, and the selection is one walk over a file's lines in order."""
import re

HEAD = re.compile(rb"([^\t\n]*)\t([0-9]{1,10})\t")
ERR_HEAD, ERR_COUNT, ERR_POS = 1, 2, 3


def lines_of(text, skip_bytes, skip_lines, at_end):
    """[(begin, end without the line break, begin of the next line)] of the complete lines behind the skip"""
    out, at = [], skip_bytes
    while True:
        nl = text.find(b"\n", at)
        if nl < 0:
            if at_end and at < len(text):
                out.append((at, len(text), len(text)))
            break
        out.append((at, nl, nl + 1))
        at = nl + 1
    return out[skip_lines:]


def head(line):
    """(CHROM, POS) of a line, or None for a malformed head"""
    m = HEAD.match(line)
    if m is None or int(m.group(2)) > 0xFFFFFFFF:
        return None
    return m.group(1), int(m.group(2))


def walk(text, lines, region):
    """one file: dict(n_lines, first, n_in, term, mal) -- mal: the line that refuses the run, or None"""
    name, beg, end = region
    first, n_in, term = None, 0, None
    for j, (a, b, _) in enumerate(lines):
        h = head(text[a:b])
        if h is None:
            return dict(n_lines=len(lines), first=0, n_in=0, term=False, mal=j)
        reached = h[0] == name and h[1] >= beg
        if first is None and reached:
            first = j
        if first is not None:
            if reached and h[1] <= end:
                n_in += 1
            else:
                term = j
                break
    return dict(n_lines=len(lines), first=len(lines) if first is None else first, n_in=n_in, term=term is not None, mal=None)


def select(texts, region, skip_bytes=None, skip_lines=None, at_end=True, max_positions=None, max_sites=None):
    """What a call takes from the files' runs: dict(P, done, err, files, rows, cursor).  err: None or (kind, file, line or
    position, second file); rows[p][f] = (begin, end) of row (p, f) in texts[f], without the line break; cursor[f] = the offset
    in texts[f] of the first byte not consumed."""
    F = len(texts)
    sb = list(skip_bytes) if skip_bytes is not None else [0] * F
    sl = list(skip_lines) if skip_lines is not None else [0] * F
    lines = [lines_of(texts[f], sb[f], sl[f], at_end) for f in range(F)]
    files = [walk(texts[f], lines[f], region) for f in range(F)]
    cap = min(x for x in (max_positions, max_sites, 1 << 32) if x is not None)
    refused = dict(P=0, done=False, files=files, rows=[], cursor=sb)
    for f in range(F):
        if files[f]["mal"] is not None:
            return dict(refused, err=(ERR_HEAD, f, files[f]["mal"], 0))
    P = min([cap] + [x["n_in"] for x in files])
    ended = [x["n_in"] == P and (x["term"] or at_end) for x in files]
    more = [x["n_in"] > P for x in files]
    if P < cap and any(ended) and any(more):
        g = ended.index(True)
        return dict(refused, err=(ERR_COUNT, g, files[g]["first"] + P, more.index(True)))
    rows = [[lines[f][files[f]["first"] + p][:2] for f in range(F)] for p in range(P)]
    for p in range(P):
        for f in range(1, F):
            if head(texts[f][slice(*rows[p][f])] + b"\n")[1] != head(texts[0][slice(*rows[p][0])] + b"\n")[1]:
                return dict(refused, err=(ERR_POS, f, p, 0))
    cursor = []
    for f in range(F):
        k = files[f]["first"] + P
        if not lines[f]:
            cursor.append(sb[f])
        elif k < len(lines[f]):
            cursor.append(lines[f][k][0])
        else:
            cursor.append(lines[f][-1][2])
    return dict(P=P, done=all(ended), err=None, files=files, rows=rows, cursor=cursor)
