"""--refresh_weights and ffm_engine_refresh_weights, the part that needs no GPU: the two entry points are
bound and refuse a null handle, the ABI version stays 4, and host/cmd_option.cpp parses the flag
(tests/refresh_weights_option_main.cpp, stand-alone; a second time under -fsanitize=address,undefined)."""
import ctypes
import os
import subprocess

import pytest

import ftrl_ffm_amd as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_bound_and_refuse_a_null_handle():
    fa.build()
    lib = fa.load_library()
    bound = {name for name, _, _ in fa.ABI}
    st = fa.engine.RefreshStats(1, 2, 3, 4, 5, 6)
    for name in ("ffm_engine_refresh_weights", "ffm_group_refresh_weights"):
        assert name in bound
        assert getattr(lib, name)(None, None) == fa.engine.E_INVALID
        assert b"null" in lib.ffm_engine_last_error()
        assert getattr(lib, name)(None, ctypes.byref(st)) == fa.engine.E_INVALID
        assert st.as_dict() == dict.fromkeys(("lin_live", "lin_nonzero", "lin_moved", "lat_live", "lat_nonzero", "lat_moved"), 0)
    assert ctypes.sizeof(fa.engine.RefreshStats) == 48
    assert lib.ffm_engine_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    assert "int ffm_engine_refresh_weights(ffm_engine *e, ffm_refresh_stats *out);" in header
    assert "int ffm_group_refresh_weights(ffm_group *g, ffm_refresh_stats *out);" in header


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_option_parsing_stand_alone(tmp_path, flags):
    exe = str(tmp_path / "refresh_weights_option")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", "refresh_weights_option_main.cpp"),
                         os.path.join(ROOT, "ftrl-ffm_amd", "host", "cmd_option.cpp")],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 13, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_cli_help_names_the_flag(tmp_path):
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin, "--refresh_weights"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--refresh_weights <bool>" in out.stderr, out.stderr
