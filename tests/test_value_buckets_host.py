"""Value buckets on the host (no GPU; include/ffm_engine.h "Value buckets"): ffm_engine_bucket_edges and
ffm_engine_bucket_ids_host -- what the device kernels are pinned to in tests/test_gpu_value_buckets.py -- against the
numpy restatement (tests/bucket_ref.py); the bucket table file of the trainer CLI, its round trip and every refusal
of a damaged one (tests/buckets_file_main.cpp); every refusal of the CLI's flags (tests/bucket_option_main.cpp)."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bucket_ref  # noqa: E402
import ftrl_ffm_amd as fa  # noqa: E402

f32 = np.float32


def _hist(val):
    return bucket_ref.np_hist(np.zeros(len(val), np.int32), np.asarray(val, f32), 1)[0][0]


def _inputs():
    rng = np.random.default_rng(1)
    heavy = np.concatenate([np.full(3000, 7.0), rng.lognormal(2.0, 2.0, 3000)])
    return {
        "random": rng.normal(0.0, 100.0, 5000),
        "lognormal": rng.lognormal(0.0, 3.0, 5000),
        "constant": np.full(1000, 3.5),
        "two-valued": np.where(rng.random(1000) < 0.3, -2.0, 11.0),
        "heavy": heavy,  # half of the mass is one value: more than 2 / B for every B >= 5
        "empty": np.zeros(0),
    }


@pytest.mark.parametrize("name", list(_inputs()))
def test_edges_are_the_reference(name):
    fa.build()
    val = np.asarray(_inputs()[name], f32)
    counts = _hist(val)
    assert int(counts.sum()) == val.size
    for B in (2, 3, 16, 32, 255, 256):
        want, dropped = bucket_ref.edges(counts, B)
        got = fa.bucket_edges(counts, B)
        assert got.dtype == np.uint16 and np.array_equal(got.astype(np.int64), want), (name, B)
        if name in ("random", "lognormal"):
            assert (B < 16 or want.size + 1 >= 3) and (B > 32 or dropped == 0), (name, B, want.size, dropped)
        if name == "heavy" and B >= 16:
            assert dropped >= 1 and want.size + 1 >= 3, "the heavy value's repeats are dropped"
        if name == "constant":
            assert want.size == 1 and dropped == B - 2
        if name == "two-valued":
            # (30 % of the mass is -2.0: its bin is an edge as soon as some j N / B <= 0.3 N, and 11.0's bin always is)
            assert want.size == (2 if B >= 4 else 1) and set(want) <= set(bucket_ref.np_bin(np.array([-2.0, 11.0], f32))[0])
        if name == "empty":
            assert want.size == 0
    for B in (1, 0, 257, -3):
        with pytest.raises(fa.EngineError) as ei:
            fa.bucket_edges(counts, B)
        assert ei.value.code == fa.engine.E_INVALID
    with pytest.raises(ValueError):
        fa.bucket_edges(counts[:100], 16)


def test_edges_with_counts_beyond_64_bit_products():
    """j * N does not fit 64 bits: the rule is still exact."""
    fa.build()
    counts = np.zeros(bucket_ref.BINS, np.uint64)
    counts[[5, 40000, 40001, 65535]] = [2 ** 62, 2 ** 61, 2 ** 62 + 12345, 2 ** 60]
    for B in (2, 7, 256):
        assert np.array_equal(fa.bucket_edges(counts, B).astype(np.int64), bucket_ref.edges(counts, B)[0]), B


def test_equal_mass():
    """What the rule is for: no bucket holds more than N / B entries plus the largest single bin."""
    fa.build()
    val = np.asarray(_inputs()["lognormal"], f32)
    counts = _hist(val).astype(np.int64)
    B = 16
    e = fa.bucket_edges(counts, B)
    assert e.size == B - 1
    per = np.bincount(bucket_ref.np_bucket(e, bucket_ref.np_bin(val)[0]), minlength=B)
    assert per.sum() == val.size and per.max() <= -(-val.size // B) + counts.max() and per.min() > 0


_BIG_DENORMAL = np.array([0x007fffff, 0x807fffff], np.uint32).view(f32)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, _BIG_DENORMAL[0], _BIG_DENORMAL[1], 3.4028235e38, -3.4028235e38,
                    1.0, -1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7, np.nan, -np.nan], f32)


def test_special_values():
    fa.build()
    b, nan = bucket_ref.np_bin(SPECIAL)
    gb, gnan = fa.value_bins(SPECIAL)
    assert np.array_equal(gnan, nan) and np.array_equal(gb[~nan], b[~nan]) and (gb[nan] == -1).all()
    assert nan.tolist() == [False] * 14 + [True, True]
    assert b[0] == b[1] == 0x8000, "+0.0 and -0.0 share a bin"
    assert b[3] == 0x007f and b[2] == 0xff80, "-inf and +inf: the outermost bins a value can have"
    assert b[4] == b[0] and b[5] == 0x7fff, "the smallest denormals: +0's bin, and the bin just below it"
    assert b[6] == 0x807f and b[7] == 0x7f80, "the largest denormals: exponent 0, the 7 mantissa bits all set"
    assert b[12] == b[10] and b[13] == b[10] + 1, "7 mantissa bits: 1 + 2^-8 shares 1.0's bin, 1 + 2^-7 does not"
    # the keys order as the values do, negatives below positives
    key, _ = bucket_ref.np_key(SPECIAL[:14])
    order = np.argsort(SPECIAL[:14].astype(np.float64), kind="stable")
    assert (np.diff(key[order].astype(np.int64)) >= 0).all()
    assert key[SPECIAL[:14] < 0].max() < key[SPECIAL[:14] >= 0].min()
    # through the library: one field whose edges are every bin named above
    edge = np.unique(b[~nan])
    assert edge.size + 1 >= 3
    feat = np.arange(SPECIAL.size, dtype=np.int32)
    got_f, got_v, hit = fa.bucket_ids(np.zeros(SPECIAL.size, np.int32), feat, SPECIAL, 1, {0: edge})
    want_f, want_v, want_hit = bucket_ref.np_apply(np.zeros(SPECIAL.size, np.int32), feat, SPECIAL, 1, {0: edge})
    assert np.array_equal(got_f, want_f) and hit.all() and want_hit.all() and (got_v == 1.0).all() and (want_v == 1.0).all()
    assert got_f[14] == got_f[15] == fa.BUCKET_NAN_ID == 65536
    assert got_f[0] == got_f[1] and got_f[3] == 0 and got_f[2] == edge.size - 1
    assert (np.diff(got_f[:14][order]) >= 0).all(), "buckets order as the values do"


@pytest.mark.parametrize("implicit", [False, True], ids=["field array", "no field array"])
def test_bucket_ids_host_is_the_reference_and_passes_the_rest_through(implicit):
    fa.build()
    F, n = 5, 4000
    rng = np.random.default_rng(7)
    field = rng.integers(0, F, n).astype(np.int32)
    feat = rng.integers(0, 2 ** 31, n, dtype=np.int64)
    val = rng.lognormal(0.0, 2.0, n).astype(f32) * np.where(rng.random(n) < 0.3, -1, 1).astype(f32)
    val[rng.random(n) < 0.3] = 2.5  # a heavy value
    val[::97] = np.nan
    val[5::101] = -0.0
    feat[3::50] = -1 - rng.integers(0, 1000, feat[3::50].size)
    if not implicit:
        field[7::60] = F
        field[9::60] = -1
    feat = feat.astype(np.int32)
    fld = None if implicit else field
    f_of = (np.arange(n) % F) if implicit else field
    table = {}
    for f in (1, 3):
        m = f_of == f
        want, dropped = bucket_ref.edges(bucket_ref.np_hist(np.zeros(int(m.sum()), np.int32), val[m], 1)[0][0], 16)
        assert want.size + 1 >= 3 and dropped >= 1, "the reference gives at least 3 buckets and drops a repeat"
        table[f] = want
    got_f, got_v, hit = fa.bucket_ids(fld, feat, val, F, table)
    want_f, want_v, want_hit = bucket_ref.np_apply(fld, feat, val, F, table)
    assert np.array_equal(got_f, want_f) and np.array_equal(hit, want_hit)
    assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32))
    # passthrough, bit for bit: negative ids, fields out of range, fields without a table
    rest = ~hit
    assert (rest & (feat < 0) & np.isin(f_of, (1, 3))).any() and (rest & ~np.isin(f_of, (1, 3))).any()
    assert implicit or ((f_of[rest] == F).any() and (f_of[rest] == -1).any())
    assert np.array_equal(got_f[rest], feat[rest]) and np.array_equal(got_v[rest].view(np.uint32), val[rest].view(np.uint32))
    assert (got_v[hit] == 1.0).all() and (got_f[hit & np.isnan(val)] == 65536).all() and (hit & np.isnan(val)).any()
    assert got_f[hit & ~np.isnan(val)].max() <= 15
    # val None: every value is 1.0
    ones_f, ones_v, _ = fa.bucket_ids(fld, feat, None, F, table)
    w_f, w_v, _ = bucket_ref.np_apply(fld, feat, np.ones(n, f32), F, table)
    assert np.array_equal(ones_f, w_f) and (ones_v == 1.0).all()
    # a field with no edges at all (N == 0): one bucket
    zero_f, _, zero_hit = fa.bucket_ids(fld, feat, val, F, {2: np.zeros(0, np.int64)})
    m = zero_hit & ~np.isnan(val)
    assert m.any() and (zero_f[m] == 0).all()


def test_table_refusals():
    fa.build()
    lib = fa.load_library()
    n_edges = np.array([-1, 2, -1], np.int32)
    edges = np.zeros((3, 255), np.uint16)
    edges[1, :2] = [9, 9]
    out_f, out_v = np.zeros(1, np.int32), np.zeros(1, f32)
    args = (1, None, out_f.ctypes.data_as(fa.engine._i32p), out_v.ctypes.data_as(fa.engine._f32p), out_f.ctypes.data_as(fa.engine._i32p),
            out_v.ctypes.data_as(fa.engine._f32p), None)
    assert lib.ffm_engine_bucket_ids_host(3, n_edges.ctypes.data, edges.ctypes.data, *args) == fa.engine.E_INVALID
    assert b"strictly ascending" in lib.ffm_engine_last_error()
    edges[1, :2] = [9, 10]
    assert lib.ffm_engine_bucket_ids_host(3, n_edges.ctypes.data, edges.ctypes.data, *args) == 0
    n_edges[2] = 256
    assert lib.ffm_engine_bucket_ids_host(3, n_edges.ctypes.data, edges.ctypes.data, *args) == fa.engine.E_INVALID
    n_edges[2] = -2
    assert lib.ffm_engine_bucket_ids_host(3, n_edges.ctypes.data, edges.ctypes.data, *args) == fa.engine.E_INVALID
    assert lib.ffm_engine_bucket_ids_host(0, n_edges.ctypes.data, edges.ctypes.data, *args) == fa.engine.E_INVALID
    assert lib.ffm_engine_bucket_ids_host(3, None, edges.ctypes.data, *args) == fa.engine.E_INVALID
    with pytest.raises(ValueError):
        fa.bucket_ids(None, out_f, out_v, 3, {3: [1]})
    with pytest.raises(ValueError):
        fa.bucket_ids(None, out_f, out_v, 3, {1: np.arange(256)})


def test_bundled_field_7():
    """The bundled file's numeric column: field 7 holds one id and thousands of distinct values."""
    fa.build()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "data", "libffm_data.txt.gz"), "rt") as f:
        toks = [tok.split(":") for line in f for tok in line.split()[1:]]
    all7 = np.array([f32(v) for fl, _, v in toks if int(fl) == 7], f32)
    val = all7[all7 != 0]  # (the parser drops zero values)
    ids = {int(i) for fl, i, v in toks if int(fl) == 7 and f32(v) != 0}
    assert len(ids) == 1 and np.unique(val).size > 1000
    counts = _hist(val)
    want, dropped = bucket_ref.edges(counts, 16)
    got = fa.bucket_edges(counts, 16)
    assert np.array_equal(got.astype(np.int64), want)
    # computed, not written down: how many entries count, how many edges the rule gives (fewer than B - 1: the column has
    # a heavy value, so repeats are dropped)
    print("field 7: %d tokens, %d zeros dropped, %d count; B = 16 gives %d edges, %d repeats dropped"
          % (all7.size, all7.size - val.size, val.size, want.size, dropped))
    assert int(counts.sum()) == val.size < all7.size and want.size + dropped == 15 and want.size + 1 >= 3 and dropped >= 1


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
def test_bucket_table_file_round_trip_and_refusals(tmp_path, flags):
    """host/value_buckets.cpp's file alone (tests/buckets_file_main.cpp): what was written is what is read; every
    corruption is refused with the path in the message."""
    exe = _compile(tmp_path, "buckets_file", "buckets_file_main.cpp", ["value_buckets.cpp"], flags)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 20, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_every_cli_refusal(tmp_path, flags):
    """--bucket_fields / --n_buckets / --buckets / --buckets_out parsed by cmd_option.cpp alone
    (tests/bucket_option_main.cpp): the defaults, what is accepted, and every refusal with its message."""
    exe = _compile(tmp_path, "bucket_option", "bucket_option_main.cpp", ["cmd_option.cpp"], flags)
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 18, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
