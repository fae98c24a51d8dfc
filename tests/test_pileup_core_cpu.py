"""CPU tests (no GPU) of the device pileup's definition, basevar_amd/csrc/bv_pileup_core.h.  The kernels of bv_pileup.hip compile
its record decode, its filter and its helpers; its walk, bv_pileup_walk, they do not: wave_walk there is the walk's second
statement, with the lanes across a match's bases, and the GPU tests hold it (test_gpu_pileup.py, test_gpu_pileup_raw.py).  Here:
the core against host/pileup.hpp on BAM files inside the stand-alone harness tests/cpp/pileup_core_check.cpp (built with ASan +
UBSan and run as a program), the harness's result against bam_py.pileup_sample, the core alone on damaged records and on every
raw run the GPU tests will send (pileup_raw_cases.py: a seeded campaign that must be worth running, and hand-built cases); the new
header against the ctypes layer; and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_py  # noqa: E402
import pileup_ref as pr  # noqa: E402
import pileup_raw_cases as rc  # noqa: E402

N_SAMPLES = 6


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from basevar_amd import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def harness(lib):
    return pr.build(asan=True)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return pr.Corpus(tmp_path_factory.mktemp("pileup_corpus"), N_SAMPLES)


def same(a, b):
    for f in ("cell", "qual", "mapq", "rank", "depth", "text"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert a.tokens.tobytes() == b.tokens.tobytes() and a.n_covered == b.n_covered


@pytest.mark.parametrize("name", sorted(pr.WINDOWS))
def test_host_core_and_independent_derivation_agree(harness, corpus, tmp_path, name):
    """the host pileup and the core, byte for byte (inside the harness), and both against bam_py.pileup_sample; the sample's records
    as one run and as a run per record"""
    window = pr.WINDOWS[name]
    d, out = pr.run_bam(harness, tmp_path / "one.bin", corpus, N_SAMPLES, window)
    assert d.status == 0 and out.startswith("status 0 ")
    assert (d.rows, d.n_samples, d.pitch, d.tid) == (window[1] - window[0] + 1, N_SAMPLES, 256, pr.TID)
    pr.check_against_bam_py(d, corpus.recs, corpus.fa, window)
    split, _ = pr.run_bam(harness, tmp_path / "split.bin", corpus, N_SAMPLES, window, split=True)
    assert split.n_runs > d.n_runs and split.records.tobytes() == d.records.tobytes()
    same(d, split)


def test_corpus_reaches_the_named_cases(harness, corpus, tmp_path):
    """what the special sample is there for does show in the planes"""
    w = pr.WINDOWS["w1000"]
    d, _ = pr.run_bam(harness, tmp_path / "a.bin", corpus, 1, w)
    tok = {int(t["pos"]): d.text[int(t["text_off"]):int(t["text_off"]) + int(t["text_len"])].tobytes().decode() for t in d.tokens}
    cell = lambda pos: int(d.cell[pos - w[0], 0])
    assert cell(1001) == "ACGT".index(corpus.recs[0][2]["seq"][100])        # the read that begins before the window
    assert cell(1056) == 4 | "ACGT".index(corpus.recs[0][3]["seq"][105])    # of two overlapping reads the first (reverse strand) won
    assert cell(1099) == 0x09 and len(tok[1099]) == 2 + 3 and int(d.rank[1099 - w[0], 0]) == 6  # I behind S claims, rank qpos + 1
    assert cell(1200) == 0x09 and tok[1200][0] == "+" and len(tok[1200]) == 4  # I then D at one break point: the I holds the anchor
    assert not any(1226 <= p <= 1250 for p in tok)                # indels behind the read's own match are refused
    assert 999 not in tok and cell(1000) < 8                      # the indel anchored before the window is not there
    assert cell(1840) == 0x0A and int(d.qual[1840 - w[0], 0]) == 255  # an empty read's indel quality
    assert cell(1264) == 0x0A | 4 and cell(1279) == 0x09 | 4 and len(tok[1279]) == 2 + 70  # an insertion longer than a wave
    assert tok[1264] == "-" + corpus.fa[1263:1266] and tok[1264][1:].islower()  # the reference's letter case is kept
    assert set(np.unique(d.cell[:, 0])) >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0x0A}
    ops = {op for r in corpus.recs[0] for op, _ in r["cigar"]}
    assert ops == set(range(9))
    # the step's edge: the last row is the last base of the step inside a read; the insertion anchored there is lost
    e = pr.WINDOWS["edge"]
    d, _ = pr.run_bam(harness, tmp_path / "e.bin", corpus, 1, e)
    assert int(d.rank[e[1] - e[0], 0]) != 0 and int(d.cell[e[1] - e[0], 0]) < 8 and all(int(t["pos"]) != 500000 for t in d.tokens)
    # the next step: the indel whose un-anchored position is its first base anchors before the window
    n = pr.WINDOWS["next"]
    d, _ = pr.run_bam(harness, tmp_path / "n.bin", corpus, 1, n)
    # (the read whose insertion was lost at the edge goes on here: its anchor lies before this window, position 500,001 is its base 33)
    assert all(int(t["pos"]) >= n[0] for t in d.tokens) and int(d.rank[0, 0]) == 30 + 2 + 1 and int(d.cell[0, 0]) & 4


def test_deletion_past_the_contigs_end_is_clipped(harness, corpus, tmp_path):
    w = (599995, 600000)
    d, _ = pr.run_bam(harness, tmp_path / "t.bin", corpus, 2, w)
    pr.check_against_bam_py(d, corpus.recs, corpus.fa, w)
    t = [t for t in d.tokens if int(t["pos"]) == 599998]
    assert len(t) == 1 and int(t[0]["text_len"]) == 2 + 2  # 20 deleted bases asked for, 2 left in the contig


def test_unknown_base_letter_gives_the_hosts_message(harness, corpus, tmp_path):
    rng = np.random.default_rng(5)
    good = pr.read(rng, 1100, [(pr.M, 40)])
    bad = pr.read(rng, 1990, [(pr.M, 40)], seq="ACGT" * 7 + "ACM" + "ACGTACGTA")  # the letter lies behind the window, inside the step
    path = str(tmp_path / "bad.bam")
    bam_py.write_bam(path, pr.REFS, [good, bad])
    d, out = pr.run_bam(harness, tmp_path / "b.bin", corpus, 1, pr.WINDOWS["w1000"], bams=[path])
    assert d.status == pr.BAD_BASE and d.fail_sample == 0
    assert "host: " + pr.BAD_BASE_TEXT + "\n" in out and out.endswith(": " + pr.BAD_BASE_TEXT + "\n")


# ------------------------------------------------------------------------------------------------------- damaged records, core only
def small_run(rng):
    return [pr.read(rng, 1000 + 3 * k, [(pr.S, 1), (pr.I, 1), (pr.M, 3)]) for k in range(3)]


def raw(harness, tmp_path, fa, runs, run_sample=None, n_samples=1, window=(1000, 1063), **kw):
    return pr.run_raw(harness, tmp_path / "r.bin", tmp_path, fa, runs, run_sample if run_sample is not None else [0] * len(runs), n_samples, window, **kw)


def test_each_refusal_has_its_status(harness, corpus, tmp_path):
    rng = np.random.default_rng(9)
    fa = corpus.fa[:4000]
    recs = [pr.record_bytes(r) for r in small_run(rng)]
    ok, out = raw(harness, tmp_path, fa, [b"".join(recs)])
    assert ok.status == 0 and ok.n_covered > 0 and ok.n_tokens == 1

    def status(run, **kw):
        d, text = raw(harness, tmp_path, kw.pop("fa", fa), [run], **kw)
        return d.status, d.fail_at, text

    patched = lambda b, at, fmt, v: b[:at] + np.array([v], fmt).tobytes() + b[at + np.dtype(fmt).itemsize:]
    r0 = recs[0]
    assert status(patched(r0, 0, "<u4", 31))[0] == pr.BAD_BLOCK                       # a block_size below 32
    assert status(recs[0] + recs[1][:-1])[:2] == (pr.BAD_RUN, len(recs[0]))          # a record that overruns its run
    assert status(recs[0] + recs[1][:3])[:2] == (pr.BAD_RUN, len(recs[0]))           # ... its block_size word does
    assert status(patched(r0, 4 + 12, "<u2", 60000))[0] == pr.BAD_LENGTHS            # n_cigar beyond the block
    assert status(patched(r0, 4 + 16, "<i4", 1 << 20))[0] == pr.BAD_LENGTHS          # l_seq beyond the block
    assert status(patched(r0, 4 + 16, "<i4", -1))[0] == pr.BAD_LENGTHS               # ... negative
    assert status(patched(r0, 4 + 8, "<u1", 255))[0] == pr.BAD_LENGTHS               # l_read_name beyond the block
    short = pr.read(rng, 1000, [(pr.M, 50)], seq="ACGTACGTAC", qual=[30] * 10)       # a CIGAR that consumes more than l_seq
    assert status(pr.record_bytes(short))[0] == pr.BAD_QUERY
    ins = pr.read(rng, 1000, [(pr.S, 20), (pr.I, 2), (pr.D, 1)], seq="ACGTACGTAC", qual=[30] * 10)  # an insertion behind the read's end
    assert status(pr.record_bytes(ins))[0] == pr.BAD_QUERY
    clipped = pr.read(rng, 1000, [(pr.S, 8), (pr.I, 5), (pr.D, 1)], seq="ACGTACGTAC", qual=[30] * 10)  # one that runs over it: clipped
    d, _ = raw(harness, tmp_path, fa, [pr.record_bytes(clipped)])
    assert d.status == 0 and d.text.tobytes() == b"+" + fa[999:1000].encode() + b"AC"
    anchor = pr.read(rng, 1040, [(pr.M, 10), (pr.N, 1), (pr.D, 5), (pr.M, 5)])        # an indel anchored outside the reference
    assert status(pr.record_bytes(anchor), fa=fa[:1045], region=(1, 1063))[0] == pr.BAD_REF
    d, _ = raw(harness, tmp_path, fa[:1052], [pr.record_bytes(anchor)], region=(1, 1063))  # deleted bases that run past its end: clipped
    assert d.status == 0 and d.text.tobytes() == b"-" + fa[1050:1052].encode()
    # a damaged record behind the one that ends the sample is never looked at; in a sample of its own it is
    far = pr.record_bytes(pr.read(rng, 5000, [(pr.M, 5)]))
    assert status(far + patched(r0, 0, "<u4", 5))[0] == 0
    d, _ = raw(harness, tmp_path, fa, [far, patched(r0, 0, "<u4", 5)], run_sample=[0, 1], n_samples=2)
    assert (d.status, d.fail_sample, d.fail_run, d.fail_at) == (pr.BAD_BLOCK, 1, 1, 0)


def test_truncation_at_every_byte_ends_in_a_status(harness, corpus, tmp_path):
    rng = np.random.default_rng(10)
    recs = [pr.record_bytes(r) for r in small_run(rng)]
    run = b"".join(recs)
    ends = set(np.cumsum([len(r) for r in recs]).tolist()) | {0}
    assert [t[1] for t in rc.truncations()] == [run[:cut] for cut in range(len(run))]  # what the GPU test sends: these bytes
    for cut in range(len(run)):
        d, _ = raw(harness, tmp_path, corpus.fa[:4000], [run[:cut]])
        assert d.status == (0 if cut in ends else pr.BAD_RUN), cut


def test_flipped_length_fields_end_in_a_status(harness, corpus, tmp_path):
    """every bit of block_size, l_read_name, n_cigar and l_seq of the middle record: a status or a clean result, no report"""
    rng = np.random.default_rng(11)
    recs = [pr.record_bytes(r) for r in small_run(rng)]
    at0 = len(recs[0])
    seen = set()
    for byte in [0, 1, 2, 3, 4 + 8, 4 + 12, 4 + 13, 4 + 16, 4 + 17, 4 + 18, 4 + 19]:
        for bit in range(8):
            run = bytearray(b"".join(recs))
            run[at0 + byte] ^= 1 << bit
            d, _ = raw(harness, tmp_path, corpus.fa[:4000], [bytes(run)])
            assert 0 <= d.status <= pr.BAD_BASE
            seen.add(d.status)
    assert {pr.BAD_BLOCK, pr.BAD_RUN, pr.BAD_LENGTHS} <= seen


# ------------------------------------------------------------------------------------------ the raw runs the GPU tests send
@pytest.fixture(scope="module")
def campaign(harness, tmp_path_factory):
    """every round of the campaign through the core under the sanitizers, once"""
    tmp = tmp_path_factory.mktemp("pileup_campaign")
    out = []
    for seed in rc.CAMPAIGN_SEEDS:
        case = rc.campaign_round(seed)
        d, text = pr.run_raw(harness, tmp / "c.bin", tmp, case[4], *case[:4])  # (raises on a sanitizer report)
        out.append((seed, case, d, text))
    return out


def test_campaign_rounds_end_clean_without_exception(campaign):
    assert 40 <= len(campaign) <= 60 and sorted(sum(rc.SEED_BLOCKS, [])) == sorted(rc.CAMPAIGN_SEEDS)
    for seed, case, d, text in campaign:
        assert d.status == 0 and text.startswith("status 0 "), seed
        assert rc.campaign_round(seed)[0] == case[0]  # seeded from the seed alone


def test_campaign_is_worth_running(campaign):
    """the GPU campaign cannot pass on nothing: tokens, coverage, every cell code, long token texts, several runs a sample; and
    what the rounds are drawn over does occur"""
    codes, longest, with_runs, several = set(), 0, 0, 0
    seen_n, seen_rows, seen_beg, first_without, last_without, short_ref, abut = set(), set(), set(), 0, 0, 0, set()
    for seed, (runs, run_sample, n, window, ref), d, _ in campaign:
        if n >= 5:
            assert d.n_tokens >= n / 4, seed
        assert d.n_covered > d.rows / 2, seed
        codes |= set(np.unique(d.cell[:, :n]).tolist())
        longest = max([longest] + d.tokens["text_len"].tolist())
        per = np.bincount(run_sample, minlength=n)
        with_runs += int((per > 0).sum())
        several += int((per > 1).sum())
        seen_n.add(n); seen_rows.add(d.rows); seen_beg.add(window[0] % 32)
        first_without += n >= 5 and per[0] == 0
        last_without += n >= 5 and per[-1] == 0
        short_ref += len(ref) < window[1] + 400
        abut |= {"first"} if window[0] == rc.GB2 else {"last"} if window[1] == rc.GB2 - 1 else set()
    assert codes >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0x0A, 0x0C, 0x0D, 0x0E}
    assert longest > 128 and any(64 < int(x) <= 128 for _, _, d, _ in campaign for x in d.tokens["text_len"])
    assert 3 * several >= with_runs
    assert seen_n == set(rc.N_SAMPLES) and seen_rows == set(rc.WINDOW_ROWS) and len(seen_beg) >= 16
    assert first_without >= 5 and last_without >= 5 and short_ref >= 5 and abut == {"first", "last"}
    assert any(len(r) == 0 for _, case, _, _ in campaign for r in case[0])  # empty runs
    assert rc.pack_is_record_bytes()


@pytest.fixture(scope="module")
def directed_dumps(harness, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pileup_directed")
    return {name: pr.run_raw(harness, tmp / (name + ".bin"), tmp, c.ref, c.runs, c.run_sample, c.n_samples, c.window)[0] for name, c in rc.directed().items()}


@pytest.mark.parametrize("name", sorted(rc.directed()))
def test_directed_case_on_the_core(directed_dumps, name):
    """no sanitizer report (run_raw raises on one), the status the case states, and its stated answer"""
    c, d = rc.directed()[name], directed_dumps[name]
    assert rc.directed_cases()[name] == c.tuple()
    assert d.status == c.status
    if c.status:
        assert (d.fail_sample, d.fail_run, d.fail_at) == c.expect["fail"]
    else:
        assert d.n_covered > 0
        rc.check_expectation(c, d)


def test_directed_cases_reach_every_status(directed_dumps):
    assert {d.status for d in directed_dumps.values()} == set(range(7))


def test_wide_and_variant_rounds_on_the_core(harness, tmp_path):
    """the many-sample rounds and the tagging boundary's reads of the GPU tests, under the sanitizers first"""
    for n in (512, 513, 1040, 4096, 4097, 4113, 20000):
        for long_rank in (8191, 8192):
            case = rc.wide_round(n, long_rank=long_rank)
            d, _ = pr.run_raw(harness, tmp_path / "w.bin", tmp_path, case[4], *case[:4])
            assert d.status == 0 and d.n_tokens > 3 and int(d.rank.max()) == long_rank == int(d.rank[-1, n - 1])
            assert sorted(set(case[1])) == case[1] and {0, 1, 63, 64, 511, n - 1} <= set(case[1]) and len(case[1]) < n // 20 + 12
    for n in (65, 4113):
        case = rc.variant_round(n)
        d, _ = pr.run_raw(harness, tmp_path / "v.bin", tmp_path, case[4], *case[:4])
        assert d.status == 0 and 250 <= d.n_covered <= 300


BAM_CASES = sorted(k for k, c in rc.directed().items() if c.recs is not None)
NOT_IN_BAM_PY = {"operation_codes_9_and_15", "insertion_of_other_nibbles"}  # bam_py knows the nine named operations and prints every letter


@pytest.mark.parametrize("name", BAM_CASES)
def test_directed_case_as_bam_files_host_against_core(harness, corpus, directed_dumps, tmp_path, name):
    """the cases that are valid BAM, written with records across BGZF members: pileup_tile against the core (inside the harness),
    one run a sample and a run a record, and both the raw case's result"""
    c = rc.directed()[name]
    bams = []
    for s, recs in enumerate(c.recs):
        bams.append(str(tmp_path / ("s%d.bam" % s)))
        bam_py.write_bam(bams[-1], pr.REFS, recs, block_payload=700)
    d, out = pr.run_bam(harness, tmp_path / "one.bin", corpus, len(bams), c.window, bams=bams)
    assert d.status == 0 and out.startswith("status 0 ")
    split, _ = pr.run_bam(harness, tmp_path / "split.bin", corpus, len(bams), c.window, split=True, bams=bams)
    assert split.n_runs >= d.n_runs
    same(d, split)
    same(d, directed_dumps[name])
    rc.check_expectation(c, d)
    if name not in NOT_IN_BAM_PY:
        pr.check_against_bam_py(d, c.recs, corpus.fa, c.window)


def test_bam_cases_are_the_ones_the_issue_names():
    assert set(BAM_CASES) >= {"no_cigar", "zero_length_operations", "quals_255_and_0", "operation_codes_9_and_15", "long_deletions", "long_insertions", "mapq_255_and_0"}


@pytest.mark.parametrize("window", [(66500, 66600), (66000, 66100)])
def test_a_read_of_66000_bases(harness, corpus, tmp_path, window):
    """query index 65,535 lies at position 66,536: its rank, 65,536, does not fit 16 bits.  The stored rank saturates at 65,535 --
    host, core and the independent derivation alike -- so the cell stays claimed and depth counts it.  (With a rank that wraps to 0
    the host counted a cell in `depth` that its row writer and the core take as unclaimed: "DIFFER: depth" on the first window.)"""
    read = rc.long_read()
    path = str(tmp_path / "long.bam")
    bam_py.write_bam(path, pr.REFS, [read])
    d, out = pr.run_bam(harness, tmp_path / "l.bin", corpus, 1, window, bams=[path])
    assert d.status == 0 and (d.depth == 1).all() and d.n_covered == d.rows
    pr.check_against_bam_py(d, [[read]], corpus.fa, window)
    want = np.minimum(np.arange(window[0], window[1] + 1) - read["pos"], 65535)
    assert (d.rank[:, 0] == want).all() and (66536 in range(window[0], window[1] + 1)) == bool((want == 65535).any())


# ---------------------------------------------------------------------------------------------------------- the header and the kernels
def test_pileup_header_symbols_are_bound_and_exported(lib):
    from basevar_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "basevar_amd_pileup.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(bv_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.PILEUP_EXPORTS) and len(names) == 6
    assert not set(names) & (set(_capi.EXPORTS) | set(_capi.BGZF_EXPORTS) | set(_capi.VCF_EXPORTS))
    for n in names:
        assert hasattr(lib, n), n
    assert lib.bv_pileup_max_rows() == pr.STEP
    for rc in (lib.bv_engine_pileup_set_reference(None, None, 0), lib.bv_engine_pileup(None, None, None, None),
               lib.bv_engine_pileup_fetch(None, None, None), lib.bv_engine_pileup_rows(None, 0, None, None, None),
               lib.bv_engine_pileup_submit(None, 0, 0, None, 0, None, None, None, None, None)):
        assert rc == _capi.BV_ERR_INVALID_ARG and b"null engine" in lib.bv_last_error(None)


def test_pileup_struct_layout_matches_header(lib, tmp_path):
    from basevar_amd import _capi
    structs = [("bv_pileup_reads", _capi.PileupReads), ("bv_pileup_result", _capi.PileupResult)]
    body = "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (n, f, n, f) for n, t in structs for f, _ in t._fields_)
    body += "".join('printf("%s.sizeof %%zu\\n", sizeof(%s));\n' % (n, n) for n, _ in structs)
    body += "".join('printf("bv_pileup_token.%s %%zu\\n", offsetof(bv_pileup_token, %s));\n' % (f, f) for f in _capi.PILEUP_TOKEN_DTYPE.names)
    body += 'printf("bv_pileup_token.sizeof %zu\\n", sizeof(bv_pileup_token));\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "basevar_amd_pileup.h"\nint main(void){\n' + body + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = dict((a, int(b)) for a, b in (l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines()))
    for n, t in structs:
        assert vals[n + ".sizeof"] == C.sizeof(t)
        for f, _ in t._fields_:
            assert vals["%s.%s" % (n, f)] == getattr(t, f).offset, (n, f)
    assert vals["bv_pileup_token.sizeof"] == _capi.PILEUP_TOKEN_DTYPE.itemsize == pr.TOKEN_DTYPE.itemsize
    for f in _capi.PILEUP_TOKEN_DTYPE.names:
        assert vals["bv_pileup_token." + f] == _capi.PILEUP_TOKEN_DTYPE.fields[f][1] == pr.TOKEN_DTYPE.fields[f][1]


def test_pileup_kernels_use_no_scratch_no_spills_and_little_lds(lib):
    """the code objects' own metadata: no private segment, no spilled register, static LDS at most 80 KiB (the `seen` bits are
    dynamic LDS: one bit a row, 62,500 bytes for bv_pileup_max_rows() rows, so two workgroups fit a CU's 160 KiB)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_scratch", os.path.join(ROOT, "tools", "kernel_scratch.py"))
    ks_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks_mod)
    if not os.path.exists(ks_mod.READELF):
        pytest.skip("llvm-readelf not found")
    from basevar_amd import _capi
    ks = [k for k in ks_mod.kernels(_capi.LIB_PATH) if "bv_pileup_" in k["name"]]
    assert len(ks) == 4  # pile, tokens, depth, gather
    for k in ks:
        assert k["private"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        assert k["lds"] <= 80 * 1024, k
    assert 2 * (4 * ((lib.bv_pileup_max_rows() + 31) // 32)) <= 160 * 1024
