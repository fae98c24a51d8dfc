"""CPU tests (no GPU) of the tabix index reader and its start query (basevar_amd/host/tabix_query.hpp) inside the stand-alone
program tests/cpp/tabix_query_check.cpp, built with ASan + UBSan: on files written through host/bgzf_tabix.hpp the query's
offset is held to tests/bam_py.py's read_tbi and a linear scan of the inflated file; the htslib-written fixture
tests/golden/chr22.all.sites.vcf.gz.tbi parses into the names, bins and linear entries read_tbi gives."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_py  # noqa: E402

SRC = os.path.join(ROOT, "tests", "cpp", "tabix_query_check.cpp")
MEMBERS = (0x300, 0x1000, 0xff00)

# positions on both sides of the 16,384 and 131,072 boundaries (a line at POS p lies in window (p - 1) >> 14), gaps of several windows
POSITIONS = {
    "cA": sorted(set(list(range(16300, 16500, 3)) + [16384, 16385] + list(range(131000, 131200, 5)) + [131072, 131073] + [1, 5, 100, 70000, 70001, 300000, 300005, 1000000])),
    "cB": [10, 20, 50000, 50001, 50002],
    "cC": [131072, 131073, 200000] + list(range(262140, 262150)),
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tabix_query") / "tabix_query_check.asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), SRC, "-lz", "-o", out])
    return out


@pytest.fixture(scope="module", params=MEMBERS)
def written(request, exe, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tbx_%x" % request.param)
    lines = os.path.join(str(tmp), "lines.txt")
    with open(lines, "wb") as o:
        for name, ps in POSITIONS.items():
            for k, p in enumerate(ps):
                o.write(b"%s\t%d\tA\t%d\t%s\n" % (name.encode(), p, k, b"q" * (320 + (k * 37) % 1600)))
    path = os.path.join(str(tmp), "x.bf.gz")
    subprocess.check_call([exe, "write", lines, str(request.param), path], stdout=subprocess.DEVNULL)
    return request.param, path


def ask(exe, tbi, queries, tmp):
    q = os.path.join(str(tmp), "queries.txt")
    with open(q, "w") as o:
        for name, beg, end in queries:
            o.write("%s %d %d\n" % (name, beg, end))
    out = subprocess.check_output([exe, "query", tbi, q]).decode().split("\n")[:-1]
    assert len(out) == len(queries)
    return [None if a == "N" else "unknown" if a == "U" else int(a.split()[1]) for a in out]


def dump(exe, tbi):
    names, refs, conf = [], [], None
    for line in subprocess.check_output([exe, "dump", tbi]).decode().split("\n")[:-1]:
        w = line.split(" ")
        if w[0] == "CONF":
            conf = tuple(int(x) for x in w[1:])
        elif w[0] == "NAME":
            names.append(w[1])
            refs.append(dict(bins={}, linear=[]))
        elif w[0] == "BIN":
            cur = refs[-1]["bins"].setdefault(int(w[1]), [])
            assert cur == [] and int(w[2]) >= 0
        elif w[0] == "CHUNK":
            cur.append((int(w[1]), int(w[2])))
        elif w[0] == "AT":
            refs[-1]["linear"].append(int(w[1]))
        else:
            assert w[0] == "LINEAR"
    return dict(conf=conf, names=names, refs=refs)


def test_reader_parses_what_read_tbi_reads(exe, written):
    member, path = written
    assert dump(exe, path + ".tbi") == bam_py.read_tbi(path + ".tbi")
    blocks = bam_py.bgzf_blocks(path)
    assert len(blocks) > {0x300: 100, 0x1000: 25, 0xff00: 3}[member] and max(len(p) for _, _, p in blocks) >= min(member, 0x300)


def test_reader_parses_the_htslib_written_fixture(exe):
    tbi = os.path.join(ROOT, "tests", "golden", "chr22.all.sites.vcf.gz.tbi")
    exp = bam_py.read_tbi(tbi)
    got = dump(exe, tbi)
    assert got == exp and got["names"] and sum(len(r["bins"]) for r in got["refs"]) > 10 and max(len(r["linear"]) for r in got["refs"]) > 10


def test_query_starts_at_or_before_the_region_and_not_before_its_window(exe, written, tmp_path):
    member, path = written
    lines = [(a, b, l.split(b"\t")[0].decode(), int(l.split(b"\t")[1])) for a, b, l in bam_py.bgzf_lines(path)]
    queries = []
    for name, ps in POSITIONS.items():
        for p in ps:
            queries += [(name, p, p), (name, p, p + 20000), (name, max(1, p - 1), p + 1), (name, p + 1, p + 1), (name, p, 1 << 29)]
        queries += [(name, 1, 1 << 29), (name, 1, 1), (name, 16384, 16384), (name, 16385, 16385), (name, 131072, 131073), (name, 20000, 60000),
                    (name, 2000000, 3000000), (name, ps[-1] + 1, 1 << 29), (name, ps[-1] + 40000, 1 << 29)]
    queries += [("cA", 6, 99), ("cA", 70002, 131000 - 1), ("cC", 1, 1000), ("cC", 1, 100000), ("cB", 21, 49999), ("cB", 30000, 32768), ("cC", 262140, 262149)]
    got = ask(exe, path + ".tbi", queries, tmp_path)
    found = nothing = between = 0
    for (name, beg, end), voff in zip(queries, got):
        mine = [(a, p) for a, b, n, p in lines if n == name]
        inside = [a for a, p in mine if beg <= p <= end]
        windows = [a for a, p in mine if (beg - 1) >> 14 <= (p - 1) >> 14 <= (min(end, 1 << 29) - 1) >> 14]
        if inside:
            assert voff is not None and voff <= inside[0], (name, beg, end)
        if windows:  # the first 16 kb window of the region that has lines: the start is its first line, or behind it
            assert voff is not None and voff >= windows[0], (name, beg, end)
            found += 1
            between += not inside
        else:
            assert voff is None, (name, beg, end)
            nothing += 1
    assert found > 100 and nothing > 10 and between > 10
    # the boundary cases by name: before all lines, behind all lines, between two lines
    by = dict(zip(queries, got))
    assert by[("cC", 1, 1000)] is None and by[("cC", 1, 100000)] is None          # before all lines, whole windows away
    assert by[("cA", 2000000, 3000000)] is None and by[("cB", 50003, 1 << 29)] is not None  # behind all lines: windows away; in the last line's window
    assert by[("cA", 6, 99)] is not None and by[("cB", 30000, 32768)] is None     # between two lines: in their window; in an empty window
    # a seek, not a scan: the last region's start lies in the file's last members
    last = [a for a, b, n, p in lines if n == "cC"][-1]
    assert by[("cC", 262140, 262149)] >> 16 > 0 and by[("cC", 262140, 262149)] <= last


def test_unknown_contig(exe, written, tmp_path):
    member, path = written
    assert ask(exe, path + ".tbi", [("cD", 1, 100), ("c", 1, 100), ("cAA", 1, 100), ("cA", 1, 100)], tmp_path)[:3] == ["unknown"] * 3
