"""FFM_FLAG_HASH_IDS on the host (no GPU): ffm_engine_hash_ids_host -- what the device kernels are pinned
to in tests/test_gpu_hash_ids.py -- against a numpy restatement of the contract in include/ffm_engine.h,
the known answers, how evenly the hash spreads, and the argument checks of a flagged create.
(The engine's switch for the flag is FFM_ENGINE_HASH_IDS; tests/test_gpu_hash_ids.py runs it.)"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ftrl_ffm_amd as fa  # noqa: E402
from hash_ref import np_hash_ids  # noqa: E402

INT32_MAX = 2 ** 31 - 1


def _entries(rng, n, n_feats, n_fields):
    feat = rng.integers(0, 2 ** 31, n, dtype=np.int64)
    feat[:8] = [0, INT32_MAX, n_feats, n_feats + 1, n_feats - 1, -1, -(2 ** 31), 1]
    feat[8:40] = rng.integers(-1000, 0, 32)
    feat[40:80] = rng.integers(n_feats, 4 * n_feats, 40)
    field = rng.integers(0, n_fields, n, dtype=np.int64)
    field[80:90] = [-1, n_fields, n_fields + 1, -7, 2 ** 31 - 1, -(2 ** 31), 0, n_fields - 1, 1000, -2]
    return field.astype(np.int32), feat.astype(np.int32)


UNEVEN = np.array([0, 7, 8, 108, 150, 203], np.int32)  # widths 7, 1 (everything maps to lo), 100, 42, 53


@pytest.mark.parametrize("fs", [None, UNEVEN], ids=["one range", "uneven field_start"])
def test_host_function_is_the_numpy_restatement_ffm(fs):
    fa.build()
    rng = np.random.default_rng(5)
    field, feat = _entries(rng, 5000, 203, 5)
    want = np_hash_ids(field, feat, 203, 5, fs, ffm=True)
    got = fa.hash_ids(field, feat, 203, field_start=fs, model="ffm", n_fields=5)
    assert np.array_equal(got, want)
    ok = want >= 0
    assert (feat[~ok] < 0).sum() > 0 and ((field[~ok] < 0) | (field[~ok] >= 5)).sum() > 0
    assert ((feat < 0) | (field < 0) | (field >= 5)).sum() == (~ok).sum(), "exactly the erased entries give -1"
    if fs is None:
        assert want[ok].min() >= 0 and want[ok].max() < 203
    else:
        f = field[ok]
        assert (want[ok] >= fs[f]).all() and (want[ok] < fs[f + 1]).all(), "every id lands in its field's range"
        assert (want[ok][f == 1] == 7).all() and (f == 1).sum() > 100, "a field of width 1 maps everything to lo"
    # implicit fields: entry p is field p mod n_fields
    got = fa.hash_ids(None, feat, 203, field_start=fs, model="ffm", n_fields=5)
    assert np.array_equal(got, np_hash_ids(None, feat, 203, 5, fs, ffm=True))
    assert np.array_equal(got, fa.hash_ids((np.arange(feat.size) % 5).astype(np.int32), feat, 203, field_start=fs, n_fields=5))


@pytest.mark.parametrize("model", ["fm", "lr"])
def test_fm_and_lr_ignore_the_field(model):
    rng = np.random.default_rng(6)
    field, feat = _entries(rng, 3000, 846153, 5)
    want = np_hash_ids(None, feat, 846153, ffm=False)
    assert np.array_equal(fa.hash_ids(field, feat, 846153, model=model), want)
    assert np.array_equal(fa.hash_ids(None, feat, 846153, model=model), want)
    assert ((want == -1) == (feat < 0)).all() and want.max() < 846153
    # (salted as field 0 of an FFM model)
    assert np.array_equal(want, np_hash_ids(np.zeros(feat.size, np.int32), feat, 846153, 1, None, ffm=True))


def test_known_answers():
    for field, feat, want in ((0, 0, 485182), (3, 12345, 487208), (38, 2147483647, 441169), (0, 1, 181360)):
        got = fa.hash_ids(np.array([field], np.int32), np.array([feat], np.int32), 846153, model="ffm", n_fields=39)
        assert int(got[0]) == want, (field, feat, int(got[0]), want)
        assert int(np_hash_ids([field], [feat], 846153, 39)[0]) == want


def test_the_hash_spreads_evenly():
    ids = np.arange(1000000, dtype=np.int32)
    worst = 0.0
    for field in (0, 1, 38):
        for width in (1000, 1024, 846153):
            h = fa.hash_ids(np.full(ids.size, field, np.int32), ids, width, model="ffm", n_fields=39)
            cnt = np.bincount(h, minlength=width).astype(np.float64)
            assert cnt.size == width
            exp = ids.size / width
            chi2_per_dof = float(((cnt - exp) ** 2 / exp).sum() / (width - 1))
            worst = max(worst, chi2_per_dof)
            assert chi2_per_dof < 1.25, (field, width, chi2_per_dof)
    print("worst chi-square per degree of freedom: %.4f" % worst)


def test_the_field_salts_the_hash():
    ids = np.arange(100000, dtype=np.int32)
    a = fa.hash_ids(np.zeros(ids.size, np.int32), ids, 1000, model="ffm", n_fields=2)
    b = fa.hash_ids(np.ones(ids.size, np.int32), ids, 1000, model="ffm", n_fields=2)
    share = float((a == b).mean())
    print("same bucket of 1000 under fields 0 and 1: %.4f %%" % (100 * share))
    assert share < 0.005, share


def test_flagged_create_refuses_a_field_of_width_zero():
    lib = fa.load_library()
    cfg = fa.Config()
    lib.ffm_engine_default_config(ctypes.byref(cfg))
    cfg.model_type, cfg.n_feats, cfg.n_fields, cfg.n_factors = 2, 203, 5, 4
    fs = np.array([0, 7, 7, 108, 150, 203], np.int32)
    cfg.field_start = fs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    cfg.flags = fa.engine.FLAG_HASH_IDS
    h = ctypes.c_void_p()
    rc = lib.ffm_engine_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == fa.engine.E_INVALID and b"width 0" in lib.ffm_engine_last_error(), (rc, lib.ffm_engine_last_error())
    assert not h.value
    # the host function refuses the same map
    with pytest.raises(fa.EngineError) as ei:
        fa.hash_ids(np.zeros(1, np.int32), np.zeros(1, np.int32), 203, field_start=fs)
    assert ei.value.code == fa.engine.E_INVALID


def test_the_abi_keeps_its_version_and_the_config_its_size():
    lib = fa.load_library()
    assert lib.ffm_engine_abi_version() == 4
    assert ctypes.sizeof(fa.Config) == 112  # (what it was before the flag: the flag lives in `flags`)
    assert fa.Config.flags.offset == 80 and fa.Config.field_start.offset == 88 and fa.Config.reserved.size == 16
    assert fa.engine.FLAG_HASH_IDS == 8
    text = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    assert "FFM_FLAG_HASH_IDS = 8" in text and "int32_t reserved[4];" in text and "#define FFM_ENGINE_ABI_VERSION 4" in text


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_hash_header_and_option_parsing_stand_alone(tmp_path, flags):
    """csrc/hash_ids.h compiled for the host alone (tests/hash_ids_host_main.cpp), and --hash_feats parsed."""
    exe = str(tmp_path / "hash_ids_host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", "hash_ids_host_main.cpp"),
                         os.path.join(ROOT, "ftrl-ffm_amd", "host", "cmd_option.cpp")],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 14, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
