"""The cases of tests/test_text_region_cpu.py: runs of short lines ("CHROM\\tPOS\\tx"), built as bytes, for the region selection of
include/basevar_amd_region.h.  A case is a dict(name, texts, region, skip_bytes, skip_lines, at_end, max_positions)."""
import random


def ln(chrom, pos, rest=b"x"):
    return chrom + b"\t" + (pos if isinstance(pos, bytes) else b"%d" % pos) + b"\t" + rest


def text(lines, last_newline=True):
    t = b"".join(l + b"\n" for l in lines)
    return t if last_newline else t[:-1]


def case(name, files, region, skip_bytes=None, skip_lines=None, at_end=True, max_positions=1000, last_newline=True):
    texts = [f if isinstance(f, bytes) else text(f, last_newline) for f in files]
    return dict(name=name, texts=texts, region=region, skip_bytes=skip_bytes or [0] * len(texts), skip_lines=skip_lines or [0] * len(texts),
                at_end=at_end, max_positions=max_positions)


# every malformed head: (label, line)
MALFORMED = [
    ("no_tab", b"c1 15 x"),
    ("one_tab", b"c1\t15"),
    ("empty_line", b""),
    ("empty_pos", b"c1\t\tx"),
    ("letter_pos", b"c1\t1a\tx"),
    ("signed_pos", b"c1\t+15\tx"),
    ("space_pos", b"c1\t15 \tx"),
    ("eleven_digits", b"c1\t00000000015\tx"),
    ("too_large", b"c1\t4294967296\tx"),
    ("pos_then_end", b"c1\t15x"),
]


def cases():
    out = []
    c1 = b"c1"
    two = [ln(c1, 5), ln(c1, 9)]
    for at_end in (True, False):
        e = "_end%d" % at_end
        out.append(case("ends_on_first" + e, [two], (c1, 1, 5), at_end=at_end))
        out.append(case("ends_on_last" + e, [two], (c1, 9, 9), at_end=at_end))
        out.append(case("ends_on_only" + e, [[ln(c1, 5)]], (c1, 5, 5), at_end=at_end))
        out.append(case("none_reached" + e, [[ln(c1, p) for p in (1, 2, 3)]], (c1, 10, 20), at_end=at_end))
        out.append(case("all_reached" + e, [[ln(c1, p) for p in (1, 2, 3)]], (c1, 1, 100), at_end=at_end))
        out.append(case("all_skipped_other_contig" + e, [[ln(b"c0", p) for p in (1, 2, 3)]], (c1, 1, 100), at_end=at_end))
        out.append(case("all_beyond" + e, [[ln(c1, p) for p in (30, 31)]], (c1, 10, 20), at_end=at_end))
    edge = [ln(c1, p) for p in (8, 9, 10, 11, 19, 20, 21, 22)]
    out.append(case("beg_and_end_edges", [edge, edge], (c1, 10, 20)))
    out.append(case("beg_minus_1_only", [[ln(c1, 9)]], (c1, 10, 20)))
    out.append(case("end_plus_1_only", [[ln(c1, 21)]], (c1, 10, 20)))
    names = [ln(b"chr", 5), ln(b"chr11", 5), ln(b"chr1", 5), ln(b"chr11", 6), ln(b"chr1", 7)]
    out.append(case("name_prefix_and_extension", [names], (b"chr1", 1, 10)))
    out.append(case("name_is_prefix_only", [names[:2] + names[3:4]], (b"chr1", 1, 10)))
    contigs = [ln(b"c0", p) for p in (1, 2, 3)] + [ln(c1, p) for p in (1, 2, 3)] + [ln(b"c2", p) for p in (1, 2, 3)]
    out.append(case("contig_before_and_behind", [contigs, contigs[2:]], (c1, 1, 1 << 29)))
    out.append(case("contig_behind_only", [contigs[3:]], (c1, 2, 3)))
    digits = [ln(c1, 5), ln(c1, 123456789), ln(c1, 1234567890), ln(c1, 4294967295)]
    out.append(case("pos_1_9_10_digits", [digits, digits], (c1, 1, 4294967295)))
    out.append(case("pos_10_digits_zero_padded", [[ln(c1, b"0000000015"), ln(c1, b"0000000016")]], (c1, 15, 15)))
    # malformed heads: in front of the region, inside it, as the line that ends it, behind the ending line
    inside = [ln(c1, p) for p in (10, 11, 12)]
    for label, bad in MALFORMED:
        out.append(case("mal_front_" + label, [[ln(c1, 1), bad] + inside + [ln(c1, 30)]], (c1, 10, 20)))
        out.append(case("mal_inside_" + label, [inside[:2] + [bad] + inside[2:] + [ln(c1, 30)]], (c1, 10, 20)))
        out.append(case("mal_ending_" + label, [inside + [bad, ln(c1, 30)]], (c1, 10, 20)))
        out.append(case("mal_behind_" + label, [inside + [ln(c1, 30), bad, ln(c1, 31)]], (c1, 10, 20)))
        out.append(case("mal_second_file_" + label, [inside + [ln(c1, 30)], inside + [bad]], (c1, 10, 20)))
        out.append(case("mal_nothing_reached_" + label, [[ln(b"c0", 1), bad, ln(b"c0", 2)]], (c1, 10, 20), at_end=False))
    seven = [ln(c1, p) for p in range(10, 17)] + [ln(c1, 40)]
    for mp in (1, 6, 7, 8, 100):
        out.append(case("max_positions_%d_n_in_7" % mp, [seven, [ln(c1, 2)] + seven], (c1, 10, 20), max_positions=mp))
    out.append(case("count_disagrees", [seven, seven[:5] + seven[7:]], (c1, 10, 20)))
    out.append(case("count_disagrees_at_end", [seven[:7], seven[:5]], (c1, 10, 20)))
    out.append(case("count_open_not_at_end", [seven[:7], seven[:5]], (c1, 10, 20), at_end=False))
    out.append(case("count_disagrees_at_cap", [seven, seven[:5] + seven[7:]], (c1, 10, 20), max_positions=5))
    out.append(case("count_disagrees_below_cap", [seven, seven[:5] + seven[7:]], (c1, 10, 20), max_positions=6))
    out.append(case("one_file_has_nothing", [seven, [ln(c1, 50)]], (c1, 10, 20)))
    out.append(case("pos_disagrees", [seven, seven[:3] + [ln(c1, 14), ln(c1, 14)] + seven[5:]], (c1, 10, 20)))
    out.append(case("pos_disagrees_third_file", [seven, seven, seven[:6] + [ln(c1, 17), ln(c1, 40)]], (c1, 10, 20)))
    out.append(case("pos_disagrees_behind_cap", [seven, seven[:3] + [ln(c1, 14), ln(c1, 14)] + seven[5:]], (c1, 10, 20), max_positions=3))
    head = [b"##a header", b"#CHROM POS"]
    out.append(case("header_lines", [head + seven, head[:1] + seven, seven], (c1, 10, 20), skip_lines=[2, 1, 0]))
    out.append(case("header_bytes_and_lines", [head + seven, b"junk" + text(head[:1] + seven)], (c1, 10, 20), skip_bytes=[len(head[0]) + 1, 4], skip_lines=[1, 1]))
    out.append(case("fewer_lines_than_header_lines", [head, seven], (c1, 10, 20), skip_lines=[3, 0], at_end=False))
    out.append(case("only_header_lines", [head, seven], (c1, 10, 20), skip_lines=[2, 0]))
    for at_end in (True, False):
        e = "_end%d" % at_end
        out.append(case("no_last_newline_inside" + e, [seven[:4]], (c1, 10, 20), at_end=at_end, last_newline=False))
        out.append(case("no_last_newline_terminating" + e, [seven], (c1, 10, 20), at_end=at_end, last_newline=False))
        out.append(case("no_last_newline_only_line" + e, [seven[:1]], (c1, 10, 20), at_end=at_end, last_newline=False))
        out.append(case("empty_file" + e, [b"", seven], (c1, 10, 20), at_end=at_end))
        out.append(case("nothing_behind_skip" + e, [text(seven[:2]), seven], (c1, 10, 20), skip_bytes=[len(text(seven[:2])), 0], at_end=at_end))
    # runs of several 16 KiB tiles: the region in the middle, beginning and ending at chosen bytes
    long_lines = [ln(c1, 1000 + p, b"y" * (p % 23)) for p in range(3000)]
    long2 = [ln(b"c0", 7)] * 5 + [ln(c1, 1000 + p, b"z" * (p % 7)) for p in range(700, 3000)]
    out.append(case("long_middle", [long_lines, long2], (c1, 2200, 3000)))
    out.append(case("long_chained_cap", [long_lines, long2], (c1, 1700, 3999), max_positions=900))
    out.append(case("long_to_the_end", [long_lines, long2], (c1, 3990, 1 << 29), at_end=False))
    out.append(case("long_chrom", [[ln(b"c" * 20000, 5), ln(b"c" * 20000 + b"d", 6), ln(b"c" * 20000, 7)]], (b"c" * 20000, 1, 10)))
    out.append(case("long_line_without_tab_behind", [[ln(c1, 10), ln(c1, 30), b"q" * 40000]], (c1, 10, 20)))
    return out + random_cases()


def random_cases(n=400, seed=20):
    rng = random.Random(seed)
    out = []
    chroms = [b"c", b"c1", b"c11", b"d"]
    for k in range(n):
        F = rng.choice((1, 1, 2, 3))
        beg = rng.randint(1, 12)
        end = beg + rng.randint(0, 8)
        base = []
        for chrom in sorted(rng.sample(chroms, rng.randint(1, 3))):
            base += [(chrom, p) for p in sorted(rng.sample(range(1, 25), rng.randint(0, 12)))]
        files, sb, sl = [], [], []
        for f in range(F):
            rows = list(base)
            r = rng.random()
            if r < 0.12 and rows:
                del rows[rng.randrange(len(rows))]
            elif r < 0.2 and rows:
                j = rng.randrange(len(rows))
                rows[j] = (rows[j][0], rows[j][1] + 1)
            lines = [ln(c, p, b"w" * rng.randint(0, 70)) for c, p in rows[rng.randint(0, 2) if rows else 0:]]
            if rng.random() < 0.08:
                lines.insert(rng.randint(0, len(lines)), rng.choice(MALFORMED)[1])
            nh = rng.choice((0, 0, 1, 3))
            lines = [b"#h%d" % i for i in range(nh)] + lines
            junk = b"j" * rng.choice((0, 0, 5))
            t = junk + text(lines, rng.random() < 0.7)
            files.append(t)
            sb.append(len(junk))
            sl.append(nh)
        out.append(case("random_%d" % k, files, (rng.choice(chroms), beg, end), skip_bytes=sb, skip_lines=sl, at_end=rng.random() < 0.5,
                        max_positions=rng.choice((1, 2, 3, 1000))))
    return out
