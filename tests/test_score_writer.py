"""Predictions as text (host/score_writer.{h,cpp} behind the CLI's --predict_out): every float is
written as the shortest decimal that parses back to the same bits, NaN and the infinities by name.
Checked without a GPU by a stand-alone program (tests/score_writer_main.cpp: 100 000 random bit
patterns, the zeros, subnormals, FLT_MAX, the infinities, NaNs) built with g++ alone, plainly and
with -fsanitize=address,undefined, and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "score_writer_main.cpp")
WRITER = os.path.join(ROOT, "ftrl-ffm_amd", "host", "score_writer.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_every_line_parses_back_to_the_same_float(tmp_path, flags):
    assert shutil.which("g++"), "g++ is needed to build the host code"
    exe = str(tmp_path / "score_writer")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags + ["-o", exe, MAIN, WRITER],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failed" in out.stdout and "FAILED" not in out.stdout, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
