"""The serving delta file format alone (host/serve_delta.{h,cpp}: ServeDeltaWriter / Reader), on the CPU:
tests/serve_delta_file_main.cpp is a stand-alone program built with g++ from persist.cpp and serve_delta.cpp
-- round trips for both formats with n_moved in {0, 1, chunk, chunk + 1}, and every rejection the reader
promises, each with the path in its message.  Built and run a second time with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "serve_delta_file_main.cpp")
SRCS = [os.path.join(ROOT, "ftrl-ffm_amd", "host", f) for f in ("persist.cpp", "serve_delta.cpp")]


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_file_format_round_trips_and_rejections(tmp_path, flags):
    assert shutil.which("g++"), "g++ is needed to build the host code"
    exe = str(tmp_path / "serve_delta_file")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags + ["-o", exe, MAIN] + SRCS + ["-ldl"],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    work = tmp_path / "files"
    work.mkdir()
    out = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout, out.stdout
    if "libzstd absent" not in out.stdout:
        assert out.stdout.count("round trip") == 8 and out.stdout.count("reject ") == 24, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
