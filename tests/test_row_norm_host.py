"""Normalised rows on the host (no GPU; include/ffm_engine.h "Normalised rows"): ffm_engine_normalize_rows_host -- the
plain C++ twin the device kernel is pinned to in tests/test_gpu_row_norm.py -- against fa.normalize_rows, the
definition in numpy, bit for bit; and --normalize_rows as cmd_option.cpp parses it (tests/row_norm_option_main.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ftrl_ffm_amd as fa  # noqa: E402

f32 = np.float32
N_FEATS, N_FIELDS = 1000, 5


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _both(row_ptr, field, feat, val, model="ffm"):
    """(numpy definition, C++ twin) of one block; asserts that they agree bit for bit."""
    fa.build()
    kw = dict(n_feats=N_FEATS, n_fields=N_FIELDS if model == "ffm" else None, model=model)
    want = fa.normalize_rows(row_ptr, field, feat, val, **kw)
    got = fa.normalize_rows_host(row_ptr, field, feat, val, **kw)
    assert want.dtype == f32 and got.dtype == f32
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    return want


def _block(lengths, rng, sigma=2.0):
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(row_ptr[-1])
    return row_ptr, rng.integers(0, N_FIELDS, n).astype(np.int32), rng.integers(0, N_FEATS, n).astype(np.int32), \
        rng.lognormal(0.0, sigma, n).astype(f32)


@pytest.mark.parametrize("model", ["ffm", "fm", "lr"])
def test_row_lengths(model):
    """Rows of 0, 1, 2, 39, 64 and 300 entries in one block, log-normal values (sigma = 2)."""
    rng = np.random.default_rng(3)
    row_ptr, field, feat, val = _block([0, 1, 2, 39, 64, 300, 0, 39], rng)
    out = _both(row_ptr, field, feat, val, model)
    for r in range(row_ptr.size - 1):
        seg = out[row_ptr[r]:row_ptr[r + 1]].astype(np.float64)
        if seg.size:
            assert abs(np.sqrt(np.sum(seg * seg)) - 1.0) < 1e-5, r


def test_the_order_of_the_sum_is_pinned():
    """2000 log-normal rows of 39 values: the host twin equals the sequential definition, and at least one row would
    come out differently under numpy's pairwise float32 sum -- so a tree order is not this definition."""
    rng = np.random.default_rng(5)
    row_ptr, field, feat, val = _block([39] * 2000, rng)
    out = _both(row_ptr, field, feat, val)
    differ = 0
    for r in range(2000):
        v = val[39 * r:39 * (r + 1)]
        s = np.sum(v * v, dtype=f32)
        tree = v * f32(f32(1.0) / np.sqrt(s))
        differ += not np.array_equal(_bits(tree), _bits(out[39 * r:39 * (r + 1)]))
    print("rows that a pairwise sum changes: %d of 2000" % differ)
    assert differ >= 1


def _rows(rows):
    """rows: lists of values, every entry kept (field 0, feat 1)."""
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    val = np.array([v for r in rows for v in r], f32)
    return row_ptr, np.zeros(val.size, np.int32), np.ones(val.size, np.int32), val


def test_edge_rows():
    """The subnormal sum, the underflowing sum, the overflowing sum, NaN, zeros and one value."""
    rows = [[1e-20, 2e-20], [1e-30], [3e19, 3e19], [np.nan, 1.0], [0.0, 0.0], [2.5], []]
    row_ptr, field, feat, val = _rows(rows)
    out = _both(row_ptr, field, feat, val)
    s = f32(f32(f32(1e-20) * f32(1e-20)) + f32(f32(2e-20) * f32(2e-20)))
    assert 0 < s < np.finfo(f32).tiny, "the sum of the first row is a subnormal"
    assert np.array_equal(out[0:2], np.array([0.44721353, 0.89442706], f32))
    assert np.array_equal(_bits(out[2:3]), _bits(val[2:3])), "1e-30: the sum underflows to 0, unchanged"
    assert np.array_equal(_bits(out[3:5]), _bits(val[3:5])), "3e19, 3e19: the sum is inf, unchanged"
    assert np.array_equal(_bits(out[5:7]), _bits(val[5:7])), "nan, 1: unchanged"
    assert np.array_equal(_bits(out[7:9]), _bits(val[7:9])), "0, 0: unchanged"
    assert out[9] == f32(1.0)


def test_erased_entries_are_left_out_of_the_sum_but_scaled():
    row_ptr = np.array([0, 5, 7], np.int32)
    field = np.array([0, 1, 2, N_FIELDS, 4, 0, -1], np.int32)
    feat = np.array([3, -1, N_FEATS, 5, 7, 1, 2], np.int32)
    val = np.array([3.0, 100.0, 200.0, 300.0, 4.0, 2.0, 50.0], f32)
    out = _both(row_ptr, field, feat, val)
    # kept: 3 and 4 (norm 5); 2 (norm 2) -- the erased entries' values are scaled by the same factor
    assert np.array_equal(out, np.array([0.6, 20.0, 40.0, 60.0, 0.8, 1.0, 25.0], f32))
    # LR / FM have no fields: the id alone decides (norm of row 0: sqrt(9 + 300^2 + 16))
    lr = _both(row_ptr, field, feat, val, "lr")
    assert lr[0] == f32(3.0) * f32(f32(1.0) / np.sqrt(f32(f32(f32(9.0) + f32(90000.0)) + f32(16.0))))
    assert lr[6] == f32(50.0) * f32(f32(1.0) / np.sqrt(f32(f32(4.0) + f32(2500.0))))
    # FFM rows without a field array: the id alone decides too
    assert np.array_equal(_bits(_both(row_ptr, None, feat, val)), _bits(lr))


def test_rows_without_values_are_rows_of_ones():
    row_ptr = np.array([0, 39, 39, 43], np.int32)
    rng = np.random.default_rng(7)
    field = rng.integers(0, N_FIELDS, 43).astype(np.int32)
    feat = rng.integers(0, N_FEATS, 43).astype(np.int32)
    out = _both(row_ptr, field, feat, None)
    assert np.array_equal(out[:39], np.full(39, 0.16012816, f32))
    assert np.array_equal(out[39:], np.full(4, 0.5, f32))
    assert np.array_equal(_bits(out), _bits(_both(row_ptr, field, feat, np.ones(43, f32))))


def test_the_twin_refuses_what_is_not_a_block():
    fa.build()
    with pytest.raises(fa.EngineError, match="n_feats must be positive"):
        fa.normalize_rows_host([0, 1], [0], [1], [1.0], n_feats=0, n_fields=2)
    with pytest.raises(ValueError, match="row_ptr"):
        fa.normalize_rows_host([0, 2, 1], [0], [1], [1.0], n_feats=4, n_fields=2)


def _compile(tmp_path, name, main, sources, flags):
    exe = str(tmp_path / name)
    host = os.path.join(ROOT, "ftrl-ffm_amd", "host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", main)] + [os.path.join(host, s) for s in sources] + ["-ldl"],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    return exe


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_cli_option(tmp_path, flags):
    """--normalize_rows parsed by cmd_option.cpp alone (tests/row_norm_option_main.cpp): the default, what is accepted,
    and the --n_gpus refusal with no device."""
    exe = _compile(tmp_path, "row_norm_option", "row_norm_option_main.cpp", ["cmd_option.cpp"], flags)
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 8, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
