#!/usr/bin/env python3
"""What does listing the batchfile rows' '+SEQ' / '-SEQ' tokens on the device cost, and what does it save?  Whole blocking calls,
wall time, through the C ABI.

    python3 tools/text_tokens_bench.py [--positions 240] [--out profiles/text_tokens_bench.txt]

Two shapes: the recorded job's (10,000 samples in 50 files) and 200 samples in 1 file, rows written from a seeded slab
(tests/test_gpu_text_rows.py: slab_rows) with 5 % of the covered calls an indel token.
  (a) bv_engine_text_parse with the mode off and on
  (b) bv_engine_text_parse_bgzf with the mode off and on
  (c) after (b) with the mode on: heads fetch + text_tokens() + indel_tally over the device tokens; after (b) with the mode off:
      rows fetch; the host walk of the marked rows (a std::string a token) and the descriptor layout, on one thread, as
      finish_text and --emit device do them (row_indel_tokens, TokenList::from_site_texts; tests/cpp/text_tokens_check.cpp `walk`, built -O2); and the tally of
      the same tokens handed in as host descriptors (the upload bv_call's default route makes).
Every figure is the best and the worst of the passes after the first, which allocates."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzf_corpus as bc  # noqa: E402
import text_tokens_model as ttm  # noqa: E402


def best_of(fn, passes=5):
    fn()
    out = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import basevar_amd as bv
    from basevar_amd import _capi
    from basevar_amd.synth import make_slab
    from test_gpu_text_rows import slab_rows
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    walk_exe = ttm.build(asan=False)
    ms = lambda t: "%.3f / %.3f ms" % (1e3 * t[0], 1e3 * t[1])  # noqa: E731
    for n_files, per in ((50, 200), (1, 200)):
        N, P, fs = n_files * per, a.positions, [per] * n_files
        slab = make_slab(P, N, seed=5, coverage=0.3, indel_frac=0.05)
        text, off = slab_rows(slab, fs)
        F = n_files
        eng = bv.BaseTypeEngine(max_sites=P, min_af_value=bv.min_af(N), device=0, max_samples=N)
        fsa = np.asarray(fs, np.uint32)
        tr = _capi.TextRows(text.ctypes.data, off.ctypes.data, fsa.ctypes.data, int(text.size), P, F, 0)
        state = np.zeros((P, F), np.uint8)

        def parse():
            assert eng._lib.bv_engine_text_parse(eng._h, C.byref(tr), None, 0, state.ctypes.data, None) == 0, eng._err()
        # the same rows as BGZF members of 0xff00 bytes, a run a file
        runs = []
        for f in range(F):
            data = b"".join(bytes(text[int(off[p * F + f]):int(off[p * F + f + 1])]) for p in range(P))
            runs.append([bc.member(data[at:at + 0xff00], 1) for at in range(0, len(data), 0xff00)])
        members = [m for run in runs for m in run]
        data = np.frombuffer(b"".join(members), np.uint8)
        moff = np.zeros(len(members) + 1, np.uint64)
        moff[1:] = np.cumsum([len(m) for m in members])
        fm = np.zeros(F + 1, np.uint32)
        fm[1:] = np.cumsum([len(r) for r in runs])
        zb, zl = np.zeros(F, np.uint64), np.zeros(F, np.uint32)
        br = _capi.BgzfRows(data.ctypes.data, moff.ctypes.data, int(data.size), fm.ctypes.data, fsa.ctypes.data, zb.ctypes.data, zl.ctypes.data, F, P, 1, 0)
        n_pos, cur = C.c_uint32(0), np.zeros((F, 2), np.uint32)

        def parse_bgzf():
            assert eng._lib.bv_engine_text_parse_bgzf(eng._h, C.byref(br), None, 0, C.byref(n_pos), state.ctypes.data, cur.ctypes.data, None) == 0, eng._err()
            assert n_pos.value == P
        say("# tools/text_tokens_bench.py: %d positions x %d samples in %d file(s), %.1f MB of rows, %.1f MB as BGZF members; best / worst of 5 passes" % (
            P, N, F, text.size / 1e6, data.size / 1e6))
        t_off, tb_off = best_of(parse), best_of(parse_bgzf)
        rows_fetch = best_of(lambda: eng.text_rows_fetch(P * F))
        rows_bytes = int(eng.text_rows_fetch(P * F)[0].size)
        eng.text_tokens_enable(True)
        t_on, tb_on = best_of(parse), best_of(parse_bgzf)
        tok, ttext = eng.text_tokens_fetch()
        key = np.nonzero((state[:, 0] & 3) == 0)[0].astype(np.uint32)  # the device-parsed positions
        marked = int(((state & 4) != 0).sum())

        def device_side():
            eng.text_heads_fetch(P * F)
            tokens, tx = eng.text_tokens()
            eng.indel_tally(key, tokens, tx)
        dev = best_of(device_side)
        heads_bytes = int(eng.text_heads_fetch(P * F)[0].size)
        host_tally = best_of(lambda: eng.indel_tally(key, tok, ttext))
        # the host route's walk and layout over the same rows, one thread
        b = ttm.Batch("bench", [[bytes(text[int(off[p * F + f]):int(off[p * F + f + 1]) - 1]) if state[p, f] & 4 else b"unmarked" for f in range(F)] for p in range(P)], fs,
                      [int(s) & 3 for s in state[:, 0]])
        with tempfile.TemporaryDirectory() as d:
            ttm.write_input(os.path.join(d, "walk.in"), [b])
            w = subprocess.run([walk_exe, "walk", os.path.join(d, "walk.in")], capture_output=True, text=True)
        assert w.returncode == 0, w.stderr
        m = re.search(r"walk: rows (\d+) tokens (\d+) text (\d+) walk_ms ([\d.]+) layout_ms ([\d.]+)", w.stdout)
        assert int(m.group(2)) == tok.size and int(m.group(3)) == ttext.size, w.stdout
        say("  tokens: %d in %d marked rows of %d (%d bytes of text); the token fetch brings %d bytes" % (tok.size, marked, P * F, ttext.size, 24 * tok.size + ttext.size))
        say("  (a) bv_engine_text_parse        mode off %s, mode on %s" % (ms(t_off), ms(t_on)))
        say("  (b) bv_engine_text_parse_bgzf   mode off %s, mode on %s" % (ms(tb_off), ms(tb_on)))
        say("  (c) heads fetch (%d bytes) + text_tokens() + tally over device tokens: %s" % (heads_bytes, ms(dev)))
        say("      rows fetch (%d bytes): %s; host walk of %s marked rows %s ms + descriptor layout %s ms (one thread, best of 5); tally of the same tokens as host descriptors: %s" % (
            rows_bytes, ms(rows_fetch), m.group(1), m.group(4), m.group(5), ms(host_tally)))
        eng.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
