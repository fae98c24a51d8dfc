"""GPU tests of `bv_call --batchfiles ... --regions R1,R2,...`: on small cohorts of indexed BGZF
batchfiles the VCF / CVG body lines of a region run are the whole-file run's lines whose (CHROM, POS) lie in the regions, in
region order -- for every combination of --inflate host|device and --emit host|device, with pop-groups, *.gz outputs,
--indel-tokens device and --devices -- and the device run seeks: it inflates fewer members.  Files without an index, plain and
plain-gzip files are scanned from their first row with a note and give the same lines."""
import gzip
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_py  # noqa: E402
from test_host_formats import cxx, make_batchfiles  # noqa: E402

ARGS = ["--contig", "chr17:81195210", "--contig", "chr18:78077248", "--reference", "hg19.fa", "--thread", "2"]
EDGE = 2515 * 16384  # a 16 kb window edge: POS EDGE is the last of window 2514, POS EDGE + 1 the first of window 2515


def place(s):
    """(CHROM, POS) of site s of make_batchfiles: chr17 across a window edge, chr17 windows further on, then chr18"""
    if s < 200:
        return "chr17", EDGE - 100 + s
    if s < 300:
        return "chr17", EDGE + 100000 + s
    return "chr18", 1000 + 3 * s


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("bin")
    exe = cxx(os.path.join(ROOT, "basevar_amd", "host", "bv_call.cpp"), str(d / "bv_call"), ["-lz"])
    writer = str(d / "tabix_query_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "tabix_query_check.cpp"),
                           "-lz", "-o", writer])
    return exe, writer


def cohort(tmp_path, writer, n_samples, n_files, members):
    """make_batchfiles' rows at place(s), written as BGZF batchfiles with a .tbi beside each; (files, sample ids, places)"""
    paths, ids, _ = make_batchfiles(tmp_path, n_sites=400, n_samples=n_samples, n_files=n_files)
    files = []
    for k, p in enumerate(paths):
        out, s = [], 0
        for line in gzip.open(p, "rb").read().split(b"\n")[:-1]:
            if line.startswith(b"#"):
                out.append(line)
                continue
            c = line.split(b"\t", 2)
            chrom, pos = place(s)
            out.append(b"%s\t%d\t%s" % (chrom.encode(), pos, c[2]))
            s += 1
        assert s == 400
        plain = str(tmp_path / ("rows_%d.txt" % k))
        open(plain, "wb").write(b"\n".join(out) + b"\n")
        q = str(tmp_path / ("cohort_%d.bf.gz" % k))
        subprocess.check_call([writer, "write", plain, str(members[k % len(members)]), q], stdout=subprocess.DEVNULL)
        files.append(q)
    return files, ids, [place(s) for s in range(400)]


def call(exe, files, tag, tmp_path, extra=(), expect=0, gz=False, inflate="device"):
    sfx = ".gz" if gz else ""
    v, c, t = str(tmp_path / (tag + ".vcf" + sfx)), str(tmp_path / (tag + ".cvg" + sfx)), str(tmp_path / (tag + ".json"))
    p = subprocess.run([exe, "--batchfiles", ",".join(files), "--output-vcf", v, "--output-cvg", c, "--timing", t, "--inflate", inflate] + ARGS + list(extra),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == expect, (p.returncode, p.stderr[-2000:])
    if expect:
        return v, c, None, p
    read = (lambda f: b"".join(pl for _, _, pl in bam_py.bgzf_blocks(f))) if gz else (lambda f: open(f, "rb").read())
    return read(v), read(c), json.load(open(t)), p


def body(text):
    return [l for l in text.split(b"\n")[:-1] if not l.startswith(b"#")]


def in_regions(lines, regions):
    """the lines whose (CHROM, POS) lie in the regions, in region order"""
    out = []
    for name, beg, end in regions:
        out += [l for l in lines if l.split(b"\t")[0] == name.encode() and beg <= int(l.split(b"\t")[1]) <= end]
    return out


def spell(regions):
    return ",".join(n if (b, e) == (1, 1 << 29) else "%s:%d" % (n, b) if e == 1 << 29 else "%s:%d-%d" % (n, b, e) for n, b, e in regions)


REGIONS = [("chr17", EDGE - 20, EDGE + 30),            # across the 16 kb window edge
           ("chr18", 1, 1 << 29),                      # a second contig, whole ("CHR")
           ("chr17", EDGE + 100250, 1 << 29),          # open-ended ("CHR:BEG"), to the end of the contig's lines
           ("chr17", EDGE + 150, EDGE + 5000),         # empty: between two lines
           ("chr17", EDGE - 100, EDGE - 100)]          # one position, the file's first row


@pytest.mark.parametrize("shape", [(180, 3), (200, 1)])
@pytest.mark.parametrize("emit", ["host", "device"])
@pytest.mark.parametrize("inflate", ["host", "device"])
def test_region_runs_give_the_whole_runs_lines_of_the_regions(tools, tmp_path, shape, emit, inflate):
    exe, writer = tools
    more0 = ["--emit", emit]

    def call(*a, **k):  # (this test's runs all take the one --inflate)
        return globals()["call"](*a, inflate=inflate, **k)
    n_samples, n_files = shape
    files, ids, places = cohort(tmp_path, writer, n_samples, n_files, (0x1000, 0x300, 0xff00))
    g = tmp_path / "groups.txt"
    g.write_text("".join("%s\tpop%02d\n" % (s, i % 2) for i, s in enumerate(ids)))
    for groups in ([], ["--pop-group", str(g)]):
        more = more0 + groups
        whole = call(exe, files, "whole", tmp_path, more)
        wv, wc = body(whole[0]), body(whole[1])
        assert len(wc) > 350 and len(wv) > 50 and "regions" not in whole[2]
        got = call(exe, files, "regions", tmp_path, more + ["--regions", spell(REGIONS)])
        assert body(got[1]) == in_regions(wc, REGIONS) and body(got[0]) == in_regions(wv, REGIONS)
        assert got[2]["regions"] == len(REGIONS) and "[NOTE]" not in got[3].stderr
        assert [h for h in got[0].split(b"\n") if h.startswith(b"#")] == [h for h in whole[0].split(b"\n") if h.startswith(b"#")]
        # every case is there: lines on both sides of the window edge, two contigs, an empty region, the one-position region
        assert len(in_regions(wc, REGIONS[:1])) > 40 and {int(l.split(b"\t")[1]) > EDGE for l in in_regions(wc, REGIONS[:1])} == {True, False}
        assert len(in_regions(wc, REGIONS[1:2])) > 80 and in_regions(wc, REGIONS[3:4]) == [] and len(in_regions(wc, REGIONS[4:])) <= 1
        assert len(in_regions(wv, REGIONS)) > 20
        # adjacent regions whose union is everything: the whole run's body, byte for byte; small batches chain a region's calls
        if groups:
            continue
        cover = [("chr17", 1, EDGE), ("chr17", EDGE + 1, EDGE + 40), ("chr17", EDGE + 41, 1 << 29), ("chr18", 1, 2000), ("chr18", 2001, 1 << 29)]
        for tag, batch in (("cover", []), ("cover7", ["--batch-sites", "7"])):
            got = call(exe, files, tag, tmp_path, more + batch + ["--regions", spell(cover)])
            assert got[0] == whole[0] and got[1] == whole[1], tag


def test_gz_outputs_hold_the_same_lines_and_their_index_finds_them(tools, tmp_path):
    exe, writer = tools
    files, ids, places = cohort(tmp_path, writer, 180, 3, (0x1000,))
    ordered = [REGIONS[4], REGIONS[0], REGIONS[3], REGIONS[2], REGIONS[1]]  # each contig's regions together and ascending
    for emit, inflate in (("host", "device"), ("device", "device"), ("host", "host"), ("device", "host")):
        tag = emit + "_" + inflate
        plain = call(exe, files, "plain_" + tag, tmp_path, ["--emit", emit, "--regions", spell(ordered)], inflate=inflate)
        got = call(exe, files, "gz_" + tag, tmp_path, ["--emit", emit, "--deflate", "device", "--regions", spell(ordered)], gz=True, inflate=inflate)
        assert got[0] == plain[0] and got[1] == plain[1] and len(body(plain[1])) > 150
        for name in ("gz_%s.vcf.gz" % tag, "gz_%s.cvg.gz" % tag):
            path = str(tmp_path / name)
            lines = [(a, l) for a, b, l in bam_py.bgzf_lines(path) if not l.startswith(b"#")]
            q = tmp_path / "q.txt"
            q.write_text("".join("%s %s %s\n" % (l.split(b"\t")[0].decode(), l.split(b"\t")[1].decode(), l.split(b"\t")[1].decode()) for a, l in lines))
            ans = subprocess.check_output([writer, "query", path + ".tbi", str(q)]).decode().split("\n")[:-1]
            assert len(ans) == len(lines) > 20
            for (a, l), x in zip(lines, ans):
                assert x.startswith("F ") and int(x.split()[1]) <= a, l[:30]


def complete_or_absent(path):
    return not os.path.exists(path) or not path.endswith(".gz") or bam_py.bgzf_blocks(path)[-1][2] == b""


def test_refusals_have_their_own_messages(tools, tmp_path):
    exe, writer = tools
    files, ids, places = cohort(tmp_path, writer, 180, 3, (0x1000,))
    cases = [("chr17:%d-%d,chr17:100-200" % (EDGE, EDGE + 10), True, "must stand together, ascending and without overlap"),
             ("chr17:100-200,chr18,chr17:%d" % EDGE, True, "must stand together, ascending and without overlap"),
             ("chr17:100-300,chr17:300-400", True, "must stand together, ascending and without overlap"),
             ("chr19:5-10", False, r"[ERROR] load data in chr19:5-10 failed. Check input file: " + files[0]),
             ("chr17:0-5", False, "wants CHR, CHR:BEG or CHR:BEG-END"),
             ("chr17:9-5", False, "wants CHR, CHR:BEG or CHR:BEG-END"),
             ("chr17:x", False, "wants CHR, CHR:BEG or CHR:BEG-END"),
             (":5-9", False, "wants CHR, CHR:BEG or CHR:BEG-END")]
    for k, (regions, gz, message) in enumerate(cases):
        v, c, _, p = call(exe, files, "bad%d" % k, tmp_path, ["--regions", regions], expect=1, gz=gz)
        assert message in p.stderr, (regions, p.stderr[-500:])
        assert complete_or_absent(v) and complete_or_absent(c)
    # out of order is fine where no index is written
    call(exe, files, "unordered", tmp_path, ["--regions", "chr18:1300-1400,chr17:%d-%d,chr18:1000-1100" % (EDGE, EDGE + 10)])
    # ... and every refusal is the same with the host reader
    for k, (regions, gz, message) in enumerate(cases):
        v, c, _, p = call(exe, files, "hbad%d" % k, tmp_path, ["--regions", regions], expect=1, gz=gz, inflate="host")
        assert message in p.stderr and complete_or_absent(v) and complete_or_absent(c)


def test_a_region_at_the_end_of_the_file_is_a_seek_not_a_scan(tools, tmp_path):
    exe, writer = tools
    files, ids, places = cohort(tmp_path, writer, 200, 1, (0x1000,))
    whole = call(exe, files, "whole", tmp_path)
    last = [("chr18", 1000 + 3 * 380, 1 << 29)]
    got = call(exe, files, "last", tmp_path, ["--regions", spell(last)])
    assert body(got[1]) == in_regions(body(whole[1]), last) and len(body(got[1])) > 10
    # the members that lie wholly before the query's offset: at least those are not inflated
    q = tmp_path / "q.txt"
    q.write_text("chr18 %d %d\n" % (last[0][1], last[0][2]))
    voff = int(subprocess.check_output([writer, "query", files[0] + ".tbi", str(q)]).decode().split()[1])
    before = sum(1 for off, size, payload in bam_py.bgzf_blocks(files[0]) if off + size <= voff >> 16)
    assert before > 50
    assert got[2]["members_inflated"] <= whole[2]["members_inflated"] - before


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_files_without_an_index_are_scanned_with_a_note(tools, tmp_path, inflate):
    exe, writer = tools
    files, ids, places = cohort(tmp_path, writer, 180, 3, (0x1000, 0x300, 0xff00))
    want = call(exe, files, "indexed", tmp_path, ["--regions", spell(REGIONS)], inflate=inflate)
    assert "[NOTE]" not in want[3].stderr
    os.remove(files[1] + ".tbi")
    got = call(exe, files, "one_scanned", tmp_path, ["--regions", spell(REGIONS)], inflate=inflate)
    assert got[0] == want[0] and got[1] == want[1] and len(body(want[1])) > 150
    assert got[3].stderr.count("[NOTE]") == 1 and "no .tbi beside " + files[1] in got[3].stderr
    for f in files:
        if os.path.exists(f + ".tbi"):
            os.remove(f + ".tbi")
    got = call(exe, files, "all_scanned", tmp_path, ["--regions", spell(REGIONS)], inflate=inflate)
    assert got[0] == want[0] and got[1] == want[1] and got[3].stderr.count("[NOTE]") == 1


def test_plain_and_plain_gzip_files_are_scanned_with_a_note(tools, tmp_path):
    """file 1 as plain text and file 2 as one plain gzip member, beside an indexed BGZF file 0: the region note names them, the
    lines are the indexed run's; --inflate device cannot take such files and says so in a note of its own"""
    exe, writer = tools
    files, ids, places = cohort(tmp_path, writer, 180, 3, (0x1000,))
    want = call(exe, files, "indexed", tmp_path, ["--regions", spell(REGIONS)], inflate="host")
    text = [b"".join(pl for _, _, pl in bam_py.bgzf_blocks(f)) for f in files]
    plain, gz = str(tmp_path / "plain_1.bf"), str(tmp_path / "gzip_2.bf.gz")
    open(plain, "wb").write(text[1])
    with gzip.open(gz, "wb") as fh:
        fh.write(text[2])
    mixed = [files[0], plain, gz]
    got = call(exe, mixed, "mixed", tmp_path, ["--regions", spell(REGIONS)], inflate="host")
    assert got[0] == want[0] and got[1] == want[1] and len(body(want[1])) > 150
    assert got[3].stderr.count("[NOTE]") == 1 and plain in got[3].stderr and gz in got[3].stderr and files[0] not in got[3].stderr
    got = call(exe, mixed, "mixed_dev", tmp_path, ["--regions", spell(REGIONS)], inflate="device")
    assert got[0] == want[0] and got[1] == want[1]
    assert got[3].stderr.count("[NOTE]") == 2 and "--inflate device needs BGZF batchfiles" in got[3].stderr


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_regions_with_indel_tokens_on_the_device_and_devices(tools, tmp_path, inflate):
    exe, writer = tools
    files, ids, places = cohort(tmp_path, writer, 180, 3, (0x1000, 0x300, 0xff00))
    want = call(exe, files, "default", tmp_path, ["--regions", spell(REGIONS)], inflate=inflate)
    assert any(b"|" in l.split(b"\t")[8] for l in body(want[1]))  # CVG rows with an indel column: the regions hold indel tokens
    for emit in ("host", "device"):
        got = call(exe, files, "tok_" + emit, tmp_path, ["--regions", spell(REGIONS), "--indel-tokens", "device", "--emit", emit, "--devices", "0"], inflate=inflate)
        assert got[0] == want[0] and got[1] == want[1]
        assert got[2]["indel_tokens"] == "device" and got[2]["indel_tokens_device"] > 0 and got[2]["regions"] == len(REGIONS)
