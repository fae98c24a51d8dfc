"""CPU test (no GPU, no engine) of bv_call's stages below the whole tool (basevar_amd/host/call_pipeline.hpp and the helpers it
shares with bv_pileup): the hand-off queue, the emitter's ordering rules -- batches finish out of order, a failed slab batch stops
everything from itself on, a failed text batch first writes its records -- the pileup window walk, region parsing, the BGZF
block table, the host's lists of indel tokens (indel_tokens.hpp) and the plan step of --emit device (device_emit.hpp).  tests/cpp/call_pipeline_check.cpp is built by g++ three ways (plain, ASan + UBSan, TSan) and each is run as a
program; nothing loaded into python runs under a sanitizer."""
import os
import subprocess

import pytest

from test_sanitize_cpu import ENV, NO_ASLR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "call_pipeline_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-pthread"]
BUILDS = {"plain": [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}


@pytest.mark.parametrize("kind", sorted(BUILDS))
def test_queue_emitter_order_window_walk_regions_and_block_table(kind, tmp_path):
    exe = str(tmp_path / ("call_pipeline_check." + kind))
    subprocess.check_call(["g++"] + FLAGS + BUILDS[kind] + [SRC, "-lz", "-o", exe])
    work = tmp_path / "out"
    work.mkdir()
    p = subprocess.run((NO_ASLR if kind == "tsan" else []) + [exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV, timeout=300)
    assert p.returncode == 0 and b"FAILS 0" in p.stdout and not p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    assert b"CALL_PIPELINE cases 124 " in p.stdout
