"""Serving engines, the part that needs no GPU: the header declares the two flags, both new functions and the
stats struct and keeps its config struct and ABI version; engine.py binds the new symbols; host/cmd_option.cpp
parses --serve_weights and refuses what a serving engine cannot do, before a device is opened
(tests/serve_option_main.cpp, stand-alone; a second time under -fsanitize=address,undefined)."""
import ctypes
import os
import re
import subprocess

import pytest

import ftrl_ffm_amd as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_feature_and_keeps_the_abi():
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    assert re.search(r"\bFFM_FLAG_SERVE_F32 = 16\b", header) and re.search(r"\bFFM_FLAG_SERVE_F16 = 32\b", header)
    assert "int ffm_engine_pack_weights(ffm_engine *dst, ffm_engine *src, ffm_pack_stats *out);" in header
    assert "int64_t ffm_engine_model_bytes(const ffm_engine *e);" in header
    assert "typedef struct { int64_t n_latent, n_inexact, n_to_inf, n_to_zero; } ffm_pack_stats;" in header
    assert "int32_t reserved[4];" in header
    assert "#define FFM_ENGINE_ABI_VERSION 4" in header
    for limit in ("FFM only", "n_shards == 1", "at most 128 entries", "No training"):
        assert limit in header, limit


def test_binding_has_the_new_symbols():
    fa.build()
    lib = fa.load_library()
    bound = {name: (res, args) for name, res, args in fa.ABI}
    assert bound["ffm_engine_pack_weights"][0] is ctypes.c_int and len(bound["ffm_engine_pack_weights"][1]) == 3
    assert bound["ffm_engine_model_bytes"][0] is ctypes.c_int64
    assert (fa.engine.FLAG_SERVE_F32, fa.engine.FLAG_SERVE_F16) == (16, 32)
    assert ctypes.sizeof(fa.engine.PackStats) == 32
    st = fa.engine.PackStats(1, 2, 3, 4)
    assert lib.ffm_engine_pack_weights(None, None, ctypes.byref(st)) == fa.engine.E_INVALID
    assert st.as_dict() == dict(n_latent=0, n_inexact=0, n_to_inf=0, n_to_zero=0)
    assert lib.ffm_engine_model_bytes(None) == 0
    assert lib.ffm_engine_abi_version() == 4
    for name in ("pack_from", "model_bytes", "load_sparse_weights", "get_weights", "set_weights"):
        assert callable(getattr(fa.Engine, name))
    with pytest.raises(ValueError):
        fa.Engine("FFM", 100, 4, 4, serve="bf16")


def test_create_refuses_bad_serving_configs_without_a_device():
    """The shape of a serving engine is checked like any argument: before a device is looked for."""
    lib = fa.load_library()

    def rc(**over):
        cfg = fa.Config()
        lib.ffm_engine_default_config(ctypes.byref(cfg))
        for k, v in over.items():
            setattr(cfg, k, v)
        h = ctypes.c_void_p()
        code = lib.ffm_engine_create(ctypes.byref(cfg), ctypes.byref(h))
        assert code != 0 or not h.value or lib.ffm_engine_destroy(h) is None
        return code, lib.ffm_engine_last_error().decode()
    assert rc(flags=16 | 32)[0] == fa.engine.E_INVALID
    assert rc(flags=32, max_row_nnz=129)[0] == fa.engine.E_INVALID
    for over in (dict(model_type=fa.FM), dict(model_type=fa.LR), dict(n_shards=2), dict(n_factors=6)):
        code, msg = rc(flags=16, **over)
        assert code == fa.engine.E_UNSUPPORTED and "serving" in msg, (over, code, msg)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_option_parsing_stand_alone(tmp_path, flags):
    exe = str(tmp_path / "serve_option")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", "serve_option_main.cpp"),
                         os.path.join(ROOT, "ftrl-ffm_amd", "host", "cmd_option.cpp")],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 21, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_cli_refuses_before_a_device_is_opened(tmp_path):
    main_bin, _ = fa.build_host()
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([main_bin, "--model_type", "FFM", "--train_data", str(data), "--serve_weights", "f16"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and out.stdout == "", out.stdout
    assert "--serve_weights f16 scores a saved model" in out.stderr and "--serve_weights <none|f32|f16>" in out.stderr
