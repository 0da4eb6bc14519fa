"""host/cmd_option.cpp's --publish_path / --publish_weights / --apply_deltas on the CPU
(tests/publish_option_main.cpp, built with g++ from cmd_option.cpp alone): the defaults are unchanged, the
accepted forms parse, every refusal comes out of parse_option before a device is opened, and the header still
says ABI version 4.  engine.py binds the four new symbols."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_publish_options(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host code"
    exe = str(tmp_path / "publish_option")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-o", exe,
                         os.path.join(ROOT, "tests", "publish_option_main.cpp"),
                         os.path.join(ROOT, "ftrl-ffm_amd", "host", "cmd_option.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    data = tmp_path / "rows.ffm"
    data.write_text("1 0:1:1 1:2:1\n0 0:3:1 1:4:0.5\n")
    work = tmp_path / "files"
    work.mkdir()
    out = subprocess.run([exe, str(data), str(work)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and out.stdout.count("refuse ") == 14, out.stdout


def test_header_and_binding_declare_the_entry_points():
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    assert re.search(r"#define FFM_ENGINE_ABI_VERSION 4\b", header)
    binding = open(os.path.join(ROOT, "ftrl-ffm_amd", "engine.py")).read()
    for name in ("ffm_engine_sync_weights", "ffm_engine_sync_moved", "ffm_engine_get_rows_raw", "ffm_engine_set_rows_raw"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert '("%s"' % name in binding, name
    assert "typedef struct { int64_t n_moved, n_lin_moved, n_lat_moved, bias_moved; } ffm_sync_stats;" in header
