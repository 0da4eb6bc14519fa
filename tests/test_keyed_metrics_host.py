"""The grouped AUC (GAUC), the part that needs no GPU: the header declares keyed capture's four functions and
its struct and keeps the ABI version; engine.py binds them; ffm_engine_metrics_from_keyed (csrc/metrics_host.h)
against fa.keyed_auc_reference -- numpy integers and a Python float loop in the header's order of operations --
bit for bit on gauc and equal on every count; the same header as a stand-alone program
(tests/keyed_metrics_host_main.cpp: g++ alone, plainly and under -fsanitize=address,undefined), which also holds
the refusals an engine's config alone decides (LR, FM, n_shards = 2, a group): ffm_engine_metrics_key_field
takes an engine, and there is no engine without a device, so the config check it calls is exercised there;
host/cmd_option.cpp's --auc_key_field / --auc_key_rows and their refusals (tests/keyed_option_main.cpp)."""
import ctypes
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ftrl_ffm_amd as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]]
COUNTS = ("n_rows", "n_keys", "n_keys_mixed", "n_rows_mixed", "n_nan", "n_unkeyed", "n_overflow")


def bits(x):
    return struct.pack("<d", x)


def test_header_and_binding_declare_the_feature_and_keep_the_abi():
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for decl in ("typedef struct { int64_t n_rows, n_keys, n_keys_mixed, n_rows_mixed, n_nan, n_unkeyed, n_overflow; double gauc; } "
                 "ffm_keyed_metrics;",
                 "int ffm_engine_metrics_key_field(ffm_engine *e, int32_t channel_mask, int32_t key_field, int64_t capacity_rows);",
                 "int ffm_engine_metrics_read_keyed(ffm_engine *e, int32_t channel, int32_t reset, ffm_keyed_metrics *out);",
                 "int ffm_engine_metrics_keyed_table(ffm_engine *e, int32_t channel, int64_t cap, int32_t *key, int64_t *pos, "
                 "int64_t *neg, uint64_t *u2, int64_t *n_keys);",
                 "int ffm_engine_metrics_from_keyed(const int64_t *pos, const int64_t *neg, const uint64_t *u2, int64_t n_keys, "
                 "ffm_keyed_metrics *out);"):
        assert decl in flat, decl
    assert "#define FFM_ENGINE_ABI_VERSION 4" in header and "int32_t reserved[4];" in header
    for said in ("is NOT captured", "merge their keys", "Out of scope", "a per-row key array passed by the caller",
                 "an exact global AUC", "engines are allowed: they predict"):
        assert said in flat, said
    bound = {n for n, _, _ in fa.ABI}
    for name in ("ffm_engine_metrics_key_field", "ffm_engine_metrics_read_keyed", "ffm_engine_metrics_keyed_table",
                 "ffm_engine_metrics_from_keyed"):
        assert name in bound, name
    assert ctypes.sizeof(fa.KeyedMetrics) == 64
    lib = fa.load_library()
    assert lib.ffm_engine_abi_version() == 4
    for method in ("metrics_key_field", "metrics_read_keyed", "metrics_keyed_table"):
        assert callable(getattr(fa.Engine, method))


def table_of(rng, n_keys, cap, mixed=0.7):
    """A random table: counts below cap, U2 anywhere in [0, 2 P N]."""
    pos = rng.integers(0, cap, n_keys).astype(np.int64)
    neg = rng.integers(0, cap, n_keys).astype(np.int64)
    pos[rng.random(n_keys) > mixed] = 0
    neg[rng.random(n_keys) > mixed] = 0
    u2 = np.array([int(rng.integers(0, 2 * int(p) * int(n) + 1, dtype=np.uint64)) if p * n else 0 for p, n in zip(pos, neg)],
                  np.uint64)
    return pos, neg, u2


def spelled(pos, neg, u2):
    """The header's order of operations over a table (what keyed_auc_reference does after its counting)."""
    num = den = 0.0
    mixed = rows_mixed = 0
    for P, N, U in zip((int(v) for v in pos), (int(v) for v in neg), (int(v) for v in u2)):
        if P == 0 or N == 0:
            continue
        num += float(P + N) * (float(U) / (2.0 * float(P) * float(N)))
        den += float(P + N)
        mixed += 1
        rows_mixed += P + N
    return dict(n_rows=int(sum(int(v) for v in pos) + sum(int(v) for v in neg)), n_keys=len(pos), n_keys_mixed=mixed,
                n_rows_mixed=rows_mixed, n_nan=0, n_unkeyed=0, n_overflow=0, gauc=num / den if den else math.nan)


def check_table(pos, neg, u2):
    got, want = fa.metrics_from_keyed(pos, neg, u2), spelled(pos, neg, u2)
    for k in COUNTS:
        assert got[k] == want[k], (k, got, want)
    assert bits(got["gauc"]) == bits(want["gauc"]) or (math.isnan(got["gauc"]) and math.isnan(want["gauc"])), (got, want)
    return got


@pytest.mark.parametrize("n_keys", [1, 2, 7, 1000, 50000])
def test_random_tables_bit_for_bit(n_keys):
    rng = np.random.default_rng(n_keys)
    for cap in (3, 1000, 1 << 20):
        check_table(*table_of(rng, n_keys, cap))


def rows_of(rng, n, n_keys, n_scores):
    keys = rng.integers(0, n_keys, n)
    p = (rng.integers(0, n_scores, n) / np.float32(n_scores)).astype(np.float32)
    return keys, p, rng.integers(-1, 2, n)


def pair_by_pair(keys, p, label, ref):
    """Every (positive, negative) pair of every key, compared as the float32 scores they are."""
    for g, key in enumerate(ref["key"]):
        sel = keys == key
        pk, yk = p[sel], label[sel] > 0
        u2 = sum(2 * int((pk[~yk] < s).sum()) + int((pk[~yk] == s).sum()) for s in pk[yk])
        assert (int(ref["pos"][g]), int(ref["neg"][g]), int(ref["u2"][g])) == (int(yk.sum()), int((~yk).sum()), u2)


def test_pair_by_pair_on_scores_an_ulp_apart_subnormals_zero_and_one():
    """The score population tests/test_gpu_keyed_sort.py relies on: float32 neighbours one ulp apart, subnormals, 0.0
    and 1.0, exact ties -- each value in both classes of one key."""
    f = np.float32
    up = lambda x: np.nextafter(f(x), f(np.inf))  # noqa: E731
    down = lambda x: np.nextafter(f(x), f(-np.inf))  # noqa: E731
    tiny = f(2.0 ** -126)
    values = np.array([0.0, up(0.0), up(up(0.0)), 1e-39, up(1e-39), down(tiny), tiny, up(tiny), 0.25, up(0.25), 0.5, down(0.5),
                       up(0.5), down(down(1.0)), down(1.0), 1.0], np.float32)
    assert np.unique(values).size == values.size == 16 and up(0.0) == f(2.0 ** -149) and (values[1:8] > 0).all()
    assert ((values > 0) & (values < tiny)).sum() == 5
    rng = np.random.default_rng(16)
    n, n_keys = 300, 3
    p = np.concatenate([np.tile(values, 2 * n_keys), rng.choice(values, n - 2 * n_keys * values.size)])
    keys = np.concatenate([np.repeat(np.arange(n_keys), 2 * values.size), rng.integers(0, n_keys, n - 2 * n_keys * values.size)])
    label = np.concatenate([np.tile(np.repeat([1, 0], values.size), n_keys), rng.integers(-1, 2, n - 2 * n_keys * values.size)])
    perm = rng.permutation(n)
    keys, p, label = keys[perm], p[perm], label[perm]
    assert p.dtype == np.float32 and p.size == n
    ref = fa.keyed_auc_reference(keys, p, label)
    assert ref["n_rows"] == n and ref["n_keys"] == ref["n_keys_mixed"] == n_keys
    pair_by_pair(keys, p, label, ref)
    got = fa.metrics_from_keyed(ref["pos"], ref["neg"], ref["u2"])
    assert bits(got["gauc"]) == bits(ref["gauc"]) and 0.0 < ref["gauc"] < 1.0
    # one ulp decides a pair: a positive moved from a tie to its upper neighbour gains exactly one half-pair
    one = fa.keyed_auc_reference([0, 0], np.array([0.25, 0.25], np.float32), [1, 0])
    two = fa.keyed_auc_reference([0, 0], np.array([up(0.25), 0.25], np.float32), [1, 0])
    sub = fa.keyed_auc_reference([0, 0], np.array([up(0.0), 0.0], np.float32), [1, 0])
    assert (one["u2"].tolist(), two["u2"].tolist(), sub["u2"].tolist()) == ([1], [2], [2])


@pytest.mark.parametrize("n,n_keys,n_scores", [(1, 1, 1), (50, 1, 3), (300, 7, 4), (5000, 40, 1000), (5000, 5000, 2), (20000, 300, 5)])
def test_rows_through_the_reference_and_the_library(n, n_keys, n_scores):
    """keyed_auc_reference counts (numpy) and averages (Python floats); the library averages the same table to
    the same bits; a pair-by-pair count agrees on the integers for the small cases."""
    rng = np.random.default_rng(n + n_keys)
    keys, p, label = rows_of(rng, n, n_keys, n_scores)
    ref = fa.keyed_auc_reference(keys, p, label)
    got = fa.metrics_from_keyed(ref["pos"], ref["neg"], ref["u2"])
    for k in COUNTS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert bits(got["gauc"]) == bits(ref["gauc"]) or (math.isnan(got["gauc"]) and math.isnan(ref["gauc"]))
    assert ref["n_rows"] == n and int(ref["pos"].sum() + ref["neg"].sum()) == n
    assert np.array_equal(ref["key"], np.unique(keys))
    if n <= 300:
        pair_by_pair(keys, p, label, ref)
    # the order the rows come in does not matter
    perm = rng.permutation(n)
    again = fa.keyed_auc_reference(keys[perm], p[perm], label[perm])
    assert bits(again["gauc"]) == bits(ref["gauc"]) or math.isnan(ref["gauc"])
    assert all(np.array_equal(again[k], ref[k]) for k in ("key", "pos", "neg", "u2"))


def test_rows_the_reference_leaves_out():
    keys = np.array([3, -1, 3, 3, 5, -7, 5])
    p = np.array([0.2, 0.9, np.nan, 0.4, 0.5, np.nan, 0.5], np.float32)
    label = np.array([0, 1, 1, 1, 0, 0, 1])
    ref = fa.keyed_auc_reference(keys, p, label)
    assert (ref["n_rows"], ref["n_nan"], ref["n_unkeyed"], ref["n_keys"], ref["n_keys_mixed"]) == (4, 2, 1, 2, 2)
    assert ref["key"].tolist() == [3, 5] and ref["u2"].tolist() == [2, 1]
    assert ref["gauc"] == (2.0 * 1.0 + 2.0 * 0.5) / 4.0


def test_no_mixed_key_is_nan_and_still_succeeds():
    m = check_table([4, 0, 2], [0, 9, 0], [0, 0, 0])
    assert math.isnan(m["gauc"]) and (m["n_keys"], m["n_keys_mixed"], m["n_rows"], m["n_rows_mixed"]) == (3, 0, 15, 0)
    m = check_table([], [], [])
    assert math.isnan(m["gauc"]) and m["n_keys"] == 0 and m["n_rows"] == 0
    ref = fa.keyed_auc_reference([1, 1, 2], np.array([0.1, 0.2, 0.3], np.float32), [1, 1, 0])
    assert math.isnan(ref["gauc"]) and ref["n_keys"] == 2 and ref["n_keys_mixed"] == 0


def test_one_key_and_all_ties():
    assert check_table([3], [5], [30])["gauc"] == 1.0
    assert check_table([3], [5], [0])["gauc"] == 0.0
    m = check_table([12], [30], [12 * 30])  # every pair a tie: U2 = P * N
    assert m["gauc"] == 0.5 and m["n_rows_mixed"] == 42
    m = check_table([12, 7, 1 << 20], [30, 7, 3], [12 * 30, 49, 3 << 20])
    assert m["gauc"] == 0.5
    ref = fa.keyed_auc_reference(np.zeros(42, np.int64), np.full(42, 0.5, np.float32), [1] * 12 + [0] * 30)
    assert ref["u2"].tolist() == [360] and ref["gauc"] == 0.5


def test_counts_near_2_to_the_31_multiply_past_63_bits():
    P, N = (1 << 31) + 5, (1 << 31) + 1
    assert 2 * P * N > 1 << 63
    m = check_table([P], [N], [P * N])
    assert abs(m["gauc"] - 0.5) < 1e-15 and m["n_rows"] == P + N
    m = check_table([P, 1], [N, 1], [2 * P * N, 0])  # U2 itself past 2^63
    assert 0.999999999 < m["gauc"] <= 1.0
    check_table([P, 7, P - 5], [N, 1, 3], [P * N + 12345, 9, (P - 5) * 5])


def test_bad_arguments():
    with pytest.raises(ValueError):
        fa.metrics_from_keyed([1, 2], [1], [1, 2])
    with pytest.raises(ValueError):
        fa.keyed_auc_reference([1, 2], np.zeros(3, np.float32), [0, 1])
    lib = fa.load_library()
    m = fa.KeyedMetrics()
    one = (ctypes.c_int64 * 1)(1)
    minus = (ctypes.c_int64 * 1)(-1)
    u = (ctypes.c_uint64 * 1)(1)
    E = fa.engine.E_INVALID
    assert lib.ffm_engine_metrics_from_keyed(one, one, u, 1, None) == E
    assert b"null" in lib.ffm_engine_last_error()
    assert lib.ffm_engine_metrics_from_keyed(None, one, u, 1, ctypes.byref(m)) == E
    assert lib.ffm_engine_metrics_from_keyed(one, None, u, 1, ctypes.byref(m)) == E
    assert lib.ffm_engine_metrics_from_keyed(one, one, None, 1, ctypes.byref(m)) == E
    assert lib.ffm_engine_metrics_from_keyed(one, one, u, -1, ctypes.byref(m)) == E
    assert lib.ffm_engine_metrics_from_keyed(minus, one, u, 1, ctypes.byref(m)) == E
    assert lib.ffm_engine_metrics_from_keyed(one, minus, u, 1, ctypes.byref(m)) == E
    assert lib.ffm_engine_metrics_from_keyed(None, None, None, 0, ctypes.byref(m)) == 0
    # without a device the engine's own calls refuse a null handle the usual way
    n = ctypes.c_int64(0)
    assert lib.ffm_engine_metrics_key_field(None, 1, 0, 100) == E
    assert lib.ffm_engine_metrics_read_keyed(None, 0, 0, ctypes.byref(m)) == E
    assert lib.ffm_engine_metrics_read_keyed(None, 0, 0, None) == E
    assert lib.ffm_engine_metrics_keyed_table(None, 0, 0, None, None, None, None, ctypes.byref(n)) == E
    assert lib.ffm_engine_metrics_keyed_table(None, 0, 0, None, None, None, None, None) == E


@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "asan_ubsan"])
def test_stand_alone_program_over_the_header(tmp_path, flags):
    assert shutil.which("g++"), "g++ is needed to build the host code"
    exe = str(tmp_path / "keyed_metrics_host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", "keyed_metrics_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failed" in out.stdout and "FAILED" not in out.stdout, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "asan_ubsan"])
def test_option_parsing_stand_alone(tmp_path, flags):
    exe = str(tmp_path / "keyed_option")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", "keyed_option_main.cpp"),
                         os.path.join(ROOT, "ftrl-ffm_amd", "host", "cmd_option.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    ffm, svm = tmp_path / "d.ffm", tmp_path / "d.svm"
    ffm.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    svm.write_text("1 1:1 7:0.5\n0 2:1 8:1\n")
    out = subprocess.run([exe, str(ffm), str(svm)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 25, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_cli_refuses_before_a_device_is_opened(tmp_path):
    main_bin, _ = fa.build_host()
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    base = [main_bin, "--model_type", "FFM", "--train_data", str(data)]
    for extra, said in ((["--auc_key_field", "0"], "it needs --metrics auc"),
                        (["--metrics", "auc", "--auc_key_field", "0", "--n_gpus", "2"], "--n_gpus > 1 is not allowed"),
                        (["--metrics", "auc", "--auc_key_field", "8"], "is not a field of this model"),
                        (["--metrics", "auc", "--auc_key_field", "0", "--auc_key_rows", "0"], "--auc_key_rows must be positive")):
        out = subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and out.stdout == "", out.stdout
        assert said in out.stderr and "--auc_key_field <F>" in out.stderr, out.stderr
