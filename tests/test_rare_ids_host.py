"""Rare ids on the host (no GPU; include/ffm_engine.h "Rare ids"): ffm_engine_fold_ids_host and
ffm_engine_rare_slots_host -- what the device kernels are pinned to in tests/test_gpu_rare_ids.py -- against the
numpy restatement (tests/rare_ref.py); the keep-map file of the trainer CLI, its round trip and every refusal of
a damaged one (tests/rare_ids_file_main.cpp); every refusal of the CLI's flags (tests/rare_option_main.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ftrl_ffm_amd as fa  # noqa: E402
import rare_ref  # noqa: E402
from hash_ref import np_hash_ids  # noqa: E402

INT32_MAX = 2 ** 31 - 1


def _entries(rng, n, n_fields):
    feat = rng.integers(0, 2 ** 31, n, dtype=np.int64)
    feat[:8] = [0, INT32_MAX, -1, -(2 ** 31), 1, 0, INT32_MAX, -1]
    feat[8:200] = rng.integers(0, 40, 192)  # repeats
    field = rng.integers(0, max(n_fields, 1), n, dtype=np.int64)
    field[:8] = [0, 0, 0, 0, -1, n_fields, max(n_fields - 1, 0), n_fields + 3]
    return field.astype(np.int32), feat.astype(np.int32)


def _map(field, feat, n_fields, bits, min_count):
    counts, _, _ = rare_ref.np_counts(field, feat, n_fields, bits, min_count)
    return rare_ref.np_keep(counts, min_count)[0]


@pytest.mark.parametrize("bits", [8, 12, 20])
def test_slots_are_the_numpy_restatement(bits):
    fa.build()
    field, feat = _entries(np.random.default_rng(bits), 3000, 5)
    ok = (feat >= 0) & (field >= 0)
    got = fa.rare_slot(field[ok], feat[ok], bits)
    assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), rare_ref.np_slot(field[ok], feat[ok], bits))
    assert got.max() < 1 << bits
    assert np.array_equal(fa.rare_slot(None, feat[ok], bits), fa.rare_slot(np.zeros(int(ok.sum()), np.int32), feat[ok], bits))
    # the slot is the top of the bits the mapping scales: with one range of 2^bits ids the model id IS the slot
    assert np.array_equal(got.astype(np.int32), np_hash_ids(field[ok], feat[ok], 1 << bits, 1 << 30))


@pytest.mark.parametrize("implicit", [False, True], ids=["field array", "no field array"])
def test_fold_is_the_numpy_restatement_ffm(implicit):
    fa.build()
    F, bits = 5, 12
    field, feat = _entries(np.random.default_rng(3), 4000, F)
    fld = None if implicit else field
    words = _map(fld, feat, F, bits, 3)
    want = rare_ref.np_fold(fld, feat, F, bits, words)
    got = fa.fold_rare(fld, feat, F, bits, words)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    ok, _ = rare_ref.np_counting(fld, feat, F)
    folded = got != feat
    assert folded.any() and (got[folded] == INT32_MAX).all() and ok[folded].all()
    assert np.array_equal(got[~ok], feat[~ok]), "erased entries stay as they are"
    assert (~folded & ok & (feat != INT32_MAX)).any(), "some entries are kept"
    if implicit:
        assert np.array_equal(got, fa.fold_rare((np.arange(feat.size) % F).astype(np.int32), feat, F, bits, words))
    # composed with the hash: erased stay erased, the rare id of a field is the model id of (field, INT32_MAX)
    fs = np.array([0, 7, 8, 108, 150, 203], np.int32)
    ids = fa.hash_ids(fld, got, 203, field_start=fs, n_fields=F)
    assert ((ids == -1) == ~ok).all()
    f_of = (np.arange(feat.size) % F) if implicit else field
    rare_of_field = fa.hash_ids(np.arange(F, dtype=np.int32), np.full(F, INT32_MAX, np.int32), 203, field_start=fs, n_fields=F)
    assert np.array_equal(ids[folded], rare_of_field[f_of[folded]])
    assert ((rare_of_field >= fs[:-1]) & (rare_of_field < fs[1:])).all(), "in the field's own range"


def test_fold_lr_takes_the_field_as_zero():
    fa.build()
    bits = 10
    field, feat = _entries(np.random.default_rng(4), 3000, 0)
    words = _map(None, feat, 0, bits, 2)
    want = rare_ref.np_fold(None, feat, 0, bits, words)
    assert np.array_equal(fa.fold_rare(None, feat, 0, bits, words), want)
    assert np.array_equal(fa.fold_rare(field, feat, 0, bits, words), want), "a field array is ignored"
    assert np.array_equal(want, rare_ref.np_fold(np.zeros(feat.size, np.int32), feat, 1, bits, words))
    assert ((want != feat) <= (feat >= 0)).all() and (want != feat).any()


def test_edge_ids_and_fields():
    fa.build()
    F, bits = 3, 8
    feat = np.array([0, -1, INT32_MAX, 0, 5, 5, -(2 ** 31), INT32_MAX], np.int32)
    field = np.array([0, 0, 1, 3, -1, 2, 2, 1], np.int32)
    none = np.zeros(4, np.uint64)
    every = np.full(4, 2 ** 64 - 1, np.uint64)
    assert np.array_equal(fa.fold_rare(field, feat, F, bits, every), feat), "a full map folds nothing"
    got = fa.fold_rare(field, feat, F, bits, none)
    assert got.tolist() == [INT32_MAX, -1, INT32_MAX, 0, 5, INT32_MAX, -(2 ** 31), INT32_MAX]
    assert np.array_equal(got, rare_ref.np_fold(field, feat, F, bits, none))
    assert fa.fold_rare(field[:0], feat[:0], F, bits, none).size == 0
    with pytest.raises(ValueError):
        fa.fold_rare(field, feat, F, bits, np.zeros(3, np.uint64))
    with pytest.raises(ValueError):
        fa.fold_rare(field, feat, F, 7, np.zeros(2, np.uint64))
    lib = fa.load_library()
    assert lib.ffm_engine_fold_ids_host(F, 31, none.ctypes.data, 0, None, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_fold_ids_host(-1, 8, none.ctypes.data, 0, None, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_fold_ids_host(F, 8, None, 0, None, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_fold_ids_host(F, 8, none.ctypes.data, 4, None, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_fold_ids_host(F, 8, none.ctypes.data, 0, None, None, None) == 0


def test_reference_keep_words_are_little_endian_bits():
    counts = np.zeros(256, np.int64)
    counts[[0, 63, 64, 255]] = [3, 2, 9, 1]
    words, kept, folded = rare_ref.np_keep(counts, 2)
    assert words.tolist() == [1 | (1 << 63), 1, 0, 0] and kept == 3 and folded == 1


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
def test_keep_map_file_round_trip_and_refusals(tmp_path, flags):
    """host/rare_ids.cpp's file alone (tests/rare_ids_file_main.cpp): what was written is what is read; a truncated
    file, a wrong checksum, another n_fields, bits that do not match the words are each refused with a message."""
    exe = _compile(tmp_path, "rare_ids_file", "rare_ids_file_main.cpp", ["rare_ids.cpp", "persist.cpp"], flags)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 16, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_every_cli_refusal(tmp_path, flags):
    """--min_count / --rare_bits / --rare_ids / --rare_ids_out parsed by cmd_option.cpp alone
    (tests/rare_option_main.cpp): the defaults, what is accepted, and every refusal with its message."""
    exe = _compile(tmp_path, "rare_option", "rare_option_main.cpp", ["cmd_option.cpp"], flags)
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 16, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
