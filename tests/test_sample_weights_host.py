"""Sample weights, the part that needs no GPU: every new entry point refuses a null engine / group with
FFM_E_INVALID, and the trainer CLI refuses bad weight flags and files before it creates an engine (on a
machine without a device the engine could not be created at all: the message must be the weights')."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ftrl_ffm_amd as fa

NEW = ["ffm_engine_train_batch_weighted", "ffm_engine_train_batch_device_weighted",
       "ffm_engine_train_forward_device_weighted", "ffm_engine_stage_batch_weighted",
       "ffm_engine_train_batch_async_weighted", "ffm_group_train_batch_weighted",
       "ffm_group_train_batch_async_weighted"]


def test_new_entry_points_are_bound_and_refuse_a_null_engine():
    fa.build()
    lib = fa.load_library()
    bound = {name: args for name, _, args in fa.ABI}
    w = np.ones(4, np.float32)
    for name in NEW:
        assert name in bound, name
        args = [None] + [0 if a in (ctypes.c_int32, ctypes.c_int) else None for a in bound[name][1:]]
        assert getattr(lib, name)(*args) == fa.engine.E_INVALID, name
        assert b"null" in lib.ffm_engine_last_error(), name
    # ... also with a weight array in hand (nothing is read through a null engine)
    fp = ctypes.POINTER(ctypes.c_float)
    assert lib.ffm_engine_train_batch_weighted(None, 4, None, None, None, None, None, w.ctypes.data_as(fp), None, None) == -1
    assert lib.ffm_engine_stage_batch_weighted(None, 4, None, None, None, None, None, w.ctypes.data, 0) == -1
    assert lib.ffm_engine_abi_version() == 4


def _cli(tmp_path, extra):
    main_bin, _ = fa.build_host()
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n\n1 0:3:1 1:9:1\n")  # three rows and a blank line
    cmd = [main_bin, "--train_data", str(data), "--model_type", "FFM", "--n_fields", "2", "--n_feats", "16",
           "--n_factors", "4"] + extra
    # (no device is asked for before the weights are read: the checks below hold with and without a GPU)
    return subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))


def test_cli_rejects_bad_class_weights_before_creating_an_engine(tmp_path):
    for flag, value in (("--neg_weight", "-1"), ("--pos_weight", "nan"), ("--pos_weight", "inf"), ("--neg_weight", "1x")):
        out = _cli(tmp_path, [flag, value])
        assert out.returncode != 0
        assert "invalid argument" in out.stderr and flag in out.stderr, out.stderr
        assert "epoch" not in out.stdout and "ffm_engine_create" not in out.stderr


def test_cli_rejects_a_short_weight_file_before_creating_an_engine(tmp_path):
    w = tmp_path / "w.txt"
    w.write_text("1\n2\n")
    out = _cli(tmp_path, ["--weight_data", str(w)])
    assert out.returncode != 0
    assert "%s:3:" % w in out.stderr and "2 weights" in out.stderr and "3 rows" in out.stderr, out.stderr
    assert "epoch" not in out.stdout and "ffm_engine_create" not in out.stderr
    w.write_text("1\n-2\n1\n")
    out = _cli(tmp_path, ["--weight_data", str(w)])
    assert out.returncode != 0 and "%s:2:" % w in out.stderr and "negative" in out.stderr, out.stderr
    assert "ffm_engine_create" not in out.stderr
    # three good weights for the three rows: the weights pass, and only then is a device asked for
    w.write_text("1\n0.5\n+2.5e0\n")
    out = _cli(tmp_path, ["--weight_data", str(w)])
    assert str(w) not in out.stderr, out.stderr


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_weight_file_reader_stand_alone(tmp_path, flags):
    """host/sample_weights.cpp alone under tests/sample_weights_file_main.cpp: every spelling the reader
    takes, every rejection with its file:line, the row count, the flags together; a second time with
    -fsanitize=address,undefined."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "sample_weights_file")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                        ["-o", exe, os.path.join(root, "tests", "sample_weights_file_main.cpp"),
                         os.path.join(root, "ftrl-ffm_amd", "host", "sample_weights.cpp")],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    work = tmp_path / "files"
    work.mkdir()
    out = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("reject ") == 16, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
