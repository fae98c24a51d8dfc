"""CPU test (no GPU) of bv_span_words, basevar_amd/csrc/bv_text_image.h: the cut of an image range into lead bytes, whole 16-byte
words and tail bytes that both device text writers store through.  tests/cpp/text_image_check.cpp includes that header alone, is
built by g++ with make sanitize's ASan + UBSan flags and run as a program; nothing loaded into python runs under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "text_image_check.cpp")
SAN_FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_every_byte_of_a_span_has_exactly_one_writer(tmp_path):
    """lo 0 .. 47 x hi lo .. lo + 96: lead, words and tail are disjoint, their union is [lo, hi), the words are whole aligned
    words, each edge has at most 15 bytes, and a range that holds no whole word has an empty word range"""
    exe = str(tmp_path / "text_image_check.asan")
    subprocess.check_call(["g++"] + SAN_FLAGS + [SRC, "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and b"FAILS 0" in p.stdout and not p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    assert b"TEXT_IMAGE cases %d " % (48 * 97) in p.stdout
