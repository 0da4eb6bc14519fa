"""Field sketches, the part that needs no GPU (include/ffm_engine.h "Field sketches"): the estimator and the range
rule against their numpy restatement (tests/sketch_ref.py); what counted ranges buy over uniform ones; the header,
the binding and the ABI list; and the CLI's --field_ranges forms, the @FILE reader and every refusal by a
stand-alone program (tests/field_ranges_main.cpp; a second time under -fsanitize=address,undefined)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ftrl_ffm_amd as fa
import hash_ref
import sketch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CARDS = (0, 1, 2, 37, 1000, 20000, 40000, 45000, 60000, 300000, 3000000)
_regs = {}


def registers(kind):
    """One sketch whose field f holds CARDS[f] distinct ids, sequential or random: built once, shared, read-only."""
    if kind not in _regs:
        rng = np.random.default_rng(20240607)
        field, feat = [], []
        for f, n in enumerate(CARDS):
            if kind == "sequential":
                ids = np.arange(n, dtype=np.int64)
            else:
                ids = np.unique(rng.integers(0, 2 ** 31, size=n + n // 8 + 8, dtype=np.int64))
                ids = rng.permutation(ids)[:n]
                assert ids.size == n
            field.append(np.full(n, f, np.int64))
            feat.append(ids)
        reg, n_valid, n_bad = sketch_ref.np_sketch(np.concatenate(field), np.concatenate(feat), len(CARDS))
        assert (n_valid, n_bad) == (sum(CARDS), 0)
        reg.setflags(write=False)
        _regs[kind] = reg
    return _regs[kind]


@pytest.mark.parametrize("kind", ["sequential", "random"])
def test_estimate_matches_the_reference_and_the_truth(kind):
    """Library against numpy: relative 1e-12 (one divide or one log away).  Against the truth: 5 % -- the
    standard error is 1.04 / sqrt(M) = 0.81 %, the uncorrected estimator's bias just above 2.5 M about 3 %."""
    fa.build()
    reg = registers(kind)
    got = fa.sketch_estimate(reg)
    want = sketch_ref.np_estimate(reg)
    assert got.dtype == np.float64 and got.shape == (len(CARDS),)
    for f, n in enumerate(CARDS):
        print("%s %8d distinct: estimate %.3f (%+.2f %%)" % (kind, n, got[f], 100.0 * (got[f] - n) / max(n, 1)))
        assert abs(got[f] - want[f]) <= 1e-12 * abs(want[f]), (n, got[f], want[f])
        assert abs(got[f] - n) <= 0.05 * n, (n, got[f])
    assert got[0] == 0.0  # an empty field


def lib_ranges(count, n_feats):
    return [int(v) for v in fa.field_ranges(np.asarray(count, np.int64), n_feats)]


EIGHT = (2, 10, 100, 1000, 10 ** 4, 10 ** 5, 3 * 10 ** 5, 10 ** 6)
RANGE_CASES = {
    "eight_fields": (EIGHT, 1 << 21),
    "all_equal": ((7,) * 5, 1000),
    "all_equal_with_remainder": ((3,) * 7, 100003),
    "one_huge": ((1, 1, 1 << 31, 1, 1), 2 ** 31 - 1),
    "huge_beyond_the_clamp": ((1, 1 << 40, 1), 1 << 20),
    "n_feats_is_twice_n_fields": ((5, 1, 9, 2), 8),
    "remainder_tie": ((1, 1, 1), 10),            # base 1, R 7: floors 2, remainders equal, one id left: field 0
    "remainder_tie_two_left": ((2, 1, 2, 1), 4 * 4096 + 10),
    "zero_counts_clamp_to_one": ((0, 0, 5, 0), 1 << 16),
    "all_zero": ((0, 0, 0), 3000),
    "one_field": ((12345,), 77),
    "thirty_nine_fields": (tuple(3 ** (f % 13) + f for f in range(39)), 33554432),
}


@pytest.mark.parametrize("name", sorted(RANGE_CASES))
def test_field_ranges_match_the_rule_exactly(name):
    fa.build()
    count, n_feats = RANGE_CASES[name]
    got = lib_ranges(count, n_feats)
    want = sketch_ref.np_field_ranges(count, n_feats)
    assert got == want, (got, want)
    width = np.diff(got)
    base = min(4096, n_feats // (2 * len(count)))
    assert got[0] == 0 and got[-1] == n_feats and int(width.sum()) == n_feats
    assert int(width.min()) >= base >= 1


def test_field_ranges_tie_goes_to_the_lower_field():
    assert lib_ranges((1, 1, 1), 10) == [0, 4, 7, 10]


def test_field_ranges_refusals():
    fa.build()
    lib = fa.load_library()
    i64p = ctypes.POINTER(ctypes.c_int64)
    i32p = ctypes.POINTER(ctypes.c_int32)
    out = np.full(5, -7, np.int32)

    def rc(count, n_fields, n_feats, null_count=False, null_out=False):
        c = np.asarray(count, np.int64)
        return lib.ffm_engine_field_ranges(None if null_count else c.ctypes.data_as(i64p), n_fields, n_feats,
                                           None if null_out else out.ctypes.data_as(i32p))
    assert rc((1, 2, 3, 4), 4, 7) == fa.engine.E_INVALID and b"2 * n_fields" in lib.ffm_engine_last_error()
    assert rc((1, 2, 3, 4), 4, 8) == 0
    assert rc((1, -1, 3, 4), 4, 100) == fa.engine.E_INVALID and b"negative count" in lib.ffm_engine_last_error()
    assert rc((1, 2), 0, 100) == fa.engine.E_INVALID
    assert rc((1, 2), -3, 100) == fa.engine.E_INVALID
    assert rc((1, 2), 2, -5) == fa.engine.E_INVALID
    assert rc((1, 2), 2, 100, null_count=True) == fa.engine.E_INVALID
    assert rc((1, 2), 2, 100, null_out=True) == fa.engine.E_INVALID
    for bad, n_feats in (((1, 2, 3, 4), 7), ((1, -1), 100)):
        with pytest.raises(fa.EngineError) as ei:
            fa.field_ranges(bad, n_feats)
        assert ei.value.code == fa.engine.E_INVALID
        with pytest.raises(ValueError):
            sketch_ref.np_field_ranges(bad, n_feats)
    # the estimator's own refusals
    f64p = ctypes.POINTER(ctypes.c_double)
    d = np.zeros(1, np.float64)
    reg = np.zeros((1, fa.engine.SKETCH_REGS), np.uint8)
    assert lib.ffm_engine_sketch_estimate(reg.ctypes.data, 0, d.ctypes.data_as(f64p)) == fa.engine.E_INVALID
    assert lib.ffm_engine_sketch_estimate(None, 1, d.ctypes.data_as(f64p)) == fa.engine.E_INVALID
    assert lib.ffm_engine_sketch_estimate(reg.ctypes.data, 1, None) == fa.engine.E_INVALID
    with pytest.raises(ValueError):
        fa.sketch_estimate(np.zeros((2, 100), np.uint8))


def test_counted_ranges_keep_more_ids_apart_than_uniform_ones():
    """Eight fields of very different cardinalities hashed into 2^21 ids with the project's own mapping: the
    ranges sized by the sketch's estimates keep strictly more distinct ids apart than uniform ranges."""
    fa.build()
    n_feats, F = 1 << 21, len(EIGHT)
    rng = np.random.default_rng(7)
    field = np.concatenate([np.full(n, f, np.int64) for f, n in enumerate(EIGHT)])
    feat = np.concatenate([rng.permutation(np.unique(rng.integers(0, 2 ** 31, size=n + n // 8 + 8, dtype=np.int64)))[:n]
                           for n in EIGHT])
    assert feat.size == sum(EIGHT)
    reg, _, _ = sketch_ref.np_sketch(field, feat, F)
    count = np.maximum(1, np.round(fa.sketch_estimate(reg))).astype(np.int64)
    counted = fa.field_ranges(count, n_feats)
    per = n_feats // F
    uniform = np.array([f * per for f in range(F)] + [n_feats], np.int32)
    kept = {}
    for name, fs in (("uniform", uniform), ("counted", counted)):
        ids = hash_ref.np_hash_ids(field, feat, n_feats, F, fs)
        assert (ids >= fs[field]).all() and (ids < fs[field + 1]).all()
        kept[name] = int(np.unique(ids).size)
    print("distinct model ids of %d raw ids: uniform %d, counted %d" % (feat.size, kept["uniform"], kept["counted"]))
    assert kept["counted"] > kept["uniform"]


def test_header_declares_the_feature_and_keeps_the_abi():
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    for decl in ("typedef struct ffm_sketch ffm_sketch;", "#define FFM_SKETCH_REGS 16384",
                 "int ffm_engine_sketch_create(int32_t n_fields, int32_t device_id, ffm_sketch **out);",
                 "int ffm_engine_sketch_add(ffm_sketch *s, int32_t nnz, const int32_t *field, const int32_t *feat, int32_t zero_copy);",
                 "int ffm_engine_sketch_add_device(ffm_sketch *s, int32_t nnz, const int32_t *field, const int32_t *feat);",
                 "int ffm_engine_sketch_read(ffm_sketch *s, uint8_t *reg",
                 "void ffm_engine_sketch_destroy(ffm_sketch *s);",
                 "int ffm_engine_sketch_estimate(const uint8_t *reg, int32_t n_fields, double *distinct",
                 "int ffm_engine_field_ranges(const int64_t *count, int32_t n_fields, int32_t n_feats, int32_t *field_start",
                 "#define FFM_ENGINE_ABI_VERSION 4"):
        assert decl in header, decl
    for words in ("Field sketches", "bijection", "no large-range correction", "OUT OF SCOPE", "ties to the lower field",
                  "rank = (w == 0) ? 19 : clz32(w) + 1", "0.7213 / (1 + 1.079 / M)"):
        assert words in header, words


NEW_SYMBOLS = ("ffm_engine_sketch_create", "ffm_engine_sketch_add", "ffm_engine_sketch_add_device", "ffm_engine_sketch_read",
               "ffm_engine_sketch_destroy", "ffm_engine_sketch_estimate", "ffm_engine_field_ranges")


def test_binding_has_the_new_symbols():
    fa.build()
    lib = fa.load_library()
    bound = {name: (res, args) for name, res, args in fa.ABI}
    for name in NEW_SYMBOLS:
        assert name in bound and hasattr(lib, name), name
        assert re.fullmatch(r"ffm_engine_\w+", name)
    assert bound["ffm_engine_sketch_destroy"][0] is None
    assert len(bound["ffm_engine_sketch_add"][1]) == 5 and len(bound["ffm_engine_sketch_read"][1]) == 4
    assert fa.engine.SKETCH_REGS == 16384 == sketch_ref.REGS
    assert lib.ffm_engine_abi_version() == 4
    for name in ("add", "add_device", "read", "estimate", "close"):
        assert callable(getattr(fa.FieldSketch, name))
    assert callable(fa.sketch_estimate) and callable(fa.field_ranges)
    # argument errors come before a device is looked for
    h = ctypes.c_void_p()
    assert lib.ffm_engine_sketch_create(0, 0, ctypes.byref(h)) == fa.engine.E_INVALID and not h.value
    assert lib.ffm_engine_sketch_create(-2, 0, ctypes.byref(h)) == fa.engine.E_INVALID
    assert lib.ffm_engine_sketch_add(None, 1, None, None, 0) == fa.engine.E_INVALID
    assert lib.ffm_engine_sketch_add_device(None, 0, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_sketch_read(None, None, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_sketch_destroy(None) is None


def test_no_sketch_without_a_gpu():
    """Without a HIP device a sketch refuses to exist (FFM_E_DEVICE): there is no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(fa.EngineError) as ei:
        fa.FieldSketch(8)
    assert ei.value.code == -2


def test_reference_inverts_the_mix():
    """sketch_ref.feat_for_bits builds the ids the GPU test needs for chosen ranks: checked against the forward mix."""
    for field, x in ((0, 0), (3, 0x0004ffff), (7, 0xfffc0000), (64, 0x12340001), (2, 0xffffffff)):
        feat = sketch_ref.feat_for_bits(field, x)
        assert -2 ** 31 <= feat < 2 ** 31
        if feat >= 0:
            assert int(sketch_ref.np_hash_bits([field], [feat])[0]) == x
    idx, rank = sketch_ref.ranks(np.array([0x00040000 - 1, 0x00040000, 0xfffe0000, 0xfffc0001, 0x00020000], np.uint64))
    assert idx.tolist() == [0, 1, 0x3fff, 0x3fff, 0]
    assert rank.tolist() == [1, 19, 1, 18, 1]


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_option_parsing_and_ranges_file_stand_alone(tmp_path, flags):
    exe = str(tmp_path / "field_ranges")
    host = os.path.join(ROOT, "ftrl-ffm_amd", "host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", "field_ranges_main.cpp"),
                         os.path.join(host, "cmd_option.cpp"), os.path.join(host, "field_ranges.cpp")],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([exe, str(data), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") >= 30, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
