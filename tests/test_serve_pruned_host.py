"""Pruned serving tables without a device: the host layout against numpy, what create refuses before a device, and what
the trainer CLI refuses for --serve_pruned true before it opens one."""
import ctypes
import subprocess

import numpy as np
import pytest

import ftrl_ffm_amd as fa

_vp, _i64p, _i32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
F32, F16, F8 = fa.engine.FLAG_SERVE_F32, fa.engine.FLAG_SERVE_F16, fa.engine.FLAG_SERVE_F8


def layout_host(words, fs):
    lib, words, fs = fa.load_library(), np.ascontiguousarray(words, np.uint64), np.ascontiguousarray(fs, np.int32)
    base = np.zeros(words.size + 1, np.int64)
    rc = lib.ffm_engine_pruned_layout_host(words.ctypes.data_as(_vp), words.size, fs.ctypes.data_as(_i32p), base.ctypes.data_as(_i64p))
    return rc, base, lib.ffm_engine_last_error().decode()


@pytest.mark.parametrize("F,n_feats", [(1, 5), (3, 9), (64, 1000), (39, 32999967)])
def test_layout_matches_its_numpy_definition(F, n_feats):
    """(39, 32 999 967) are the headline numbers: under a quarter mask the element offsets pass 2^31."""
    words = fa.pair_mask(F, list(zip(*np.nonzero(np.triu(np.random.default_rng(F).random((F, F)) < 0.25)))))
    fs = np.round(np.linspace(0, n_feats, F + 1)).astype(np.int32)
    rc, base, msg = layout_host(words, fs)
    want, P = fa.pruned_layout(words, fs)
    assert rc == 0 and np.array_equal(base, want) and want[-1] == int((np.diff(fs.astype(np.int64)) * P).sum()), msg
    if n_feats > 1 << 24:
        assert (1 << 31) // 16 < want[-1] < 1 << 32 and want[-1] < n_feats * F // 2


def create_rc(words, n_fields=3, flags=F16, fs=(0, 4, 8, 12)):
    lib, cfg = fa.load_library(), fa.Config()
    lib.ffm_engine_default_config(ctypes.byref(cfg))
    cfg.n_feats, cfg.n_fields, cfg.n_factors, cfg.max_batch_rows, cfg.max_batch_nnz, cfg.flags = 12, 3, 4, 16, 1024, flags
    if fs is not None:
        fs = np.array(fs, np.int32)
        cfg.field_start = fs.ctypes.data_as(_i32p)
    h, words = ctypes.c_void_p(), np.ascontiguousarray(words, np.uint64)
    rc = lib.ffm_engine_create_pruned(ctypes.byref(cfg), words.ctypes.data_as(_vp), n_fields, ctypes.byref(h))
    assert rc != 0, "refused before a device is opened"
    return rc, lib.ffm_engine_last_error().decode()


REFUSALS = {  # the mask messages are ffm_engine_set_pair_mask's own (tests/test_gpu_pair_mask.py pins them there)
    "asymmetric": (dict(words=[2, 0, 0]), -1, "the mask is not symmetric: bit 0 of keep[1] differs from bit 1 of keep[0]"),
    "a bit above": (dict(words=[8, 0, 0]), -1, "keep[0] has a bit at or above n_fields"),
    "other n_fields": (dict(words=[3, 3], n_fields=2), -1, "the mask is for 2 fields, the engine has 3"),
    "f8": (dict(words=[7, 7, 7], flags=F8), -5, "FFM_FLAG_SERVE_F8"),
    "no format": (dict(words=[7, 7, 7], flags=0), -1, "FFM_FLAG_SERVE_F32 or FFM_FLAG_SERVE_F16"),
    "both formats": (dict(words=[7, 7, 7], flags=F32 | F16), -1, "exclude each other"),
    "no ranges": (dict(words=[7, 7, 7], fs=None), -1, "field_start == NULL"),
    "ranges short of n_feats": (dict(words=[7, 7, 7], fs=(0, 4, 8, 11)), -1, "field_start must ascend from 0 to n_feats"),
    "descending ranges": (dict(words=[7, 7, 7], fs=(0, 8, 4, 12)), -1, "field_start must ascend from 0 to n_feats"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refused_before_a_device_is_opened(name):
    kw, code, text = REFUSALS[name]
    rc, msg = create_rc(**kw)
    assert rc == code and text in msg, (rc, msg)


def test_layout_refuses_what_create_refuses():
    rc, _, msg = layout_host([1] * 65, np.arange(66))
    assert rc == -5 and "at most 64 fields" in msg
    # 2^32 slots or more: 64 fields of 2^25 ids with every partner kept
    rc, _, msg = layout_host([2 ** 64 - 1] * 64, np.arange(65, dtype=np.int64) * (1 << 25) - np.arange(65) // 64)
    assert rc == -5 and "2^32" in msg


CLI = ["--model_type", "FFM", "--n_fields", "4", "--n_feats", "400", "--n_factors", "4", "--resume_from", "ck", "--n_epochs", "0", "--eval_data",
       "d.ffm", "--serve_pruned", "true", "--serve_weights", "f16", "--pair_mask", "@mask.txt", "--hash_feats", "true", "--field_ranges", "uniform"]
CLI_REFUSALS = {  # name: (flags dropped, flags added, what the first line of stderr names beside --serve_pruned)
    "f8": (["--serve_weights"], ["--serve_weights", "f8"], "--serve_weights f8"),
    "no serving format": (["--serve_weights"], [], "--serve_weights"),
    "no mask": (["--pair_mask"], [], "--pair_mask"),
    "deltas": (["--resume_from"], ["--apply_deltas", "P"], "--apply_deltas"),
    "pair importance": ([], ["--pair_importance", "true"], "--pair_importance"),
    "field importance": ([], ["--field_importance", "true"], "--field_importance"),
    "ids not hashed": (["--hash_feats"], [], "--hash_feats"),
    "no ranges": (["--field_ranges"], [], "--field_ranges"),
    "fewer ids than fields": (["--n_feats"], ["--n_feats", "3"], "--n_feats"),
}


@pytest.mark.parametrize("name", sorted(CLI_REFUSALS))
def test_the_cli_refuses_before_it_opens_a_device(tmp_path, name):
    drop, add, named = CLI_REFUSALS[name]
    args = [a for i, a in enumerate(CLI) if a not in drop and (i == 0 or CLI[i - 1] not in drop)] + add
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    first = out.stderr.split("\n")[0]
    assert out.returncode != 0 and "--serve_pruned" in first and named in first, out.stderr[:300]
    assert out.stdout == ""  # (nothing is printed: no file was read and no device opened)
