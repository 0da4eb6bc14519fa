"""Pair ablation, the part that needs no GPU (include/ffm_engine.h "Pair ablation"): the numbering of the variants,
C against numpy, for every n_fields in 1 .. 64; the zeroed-slot argument that the GPU tests rest on, checked on the
oracle alone; the header declares the entry points and keeps its ABI version, the library exports them; the CLI
flag, its refusals and host/importance.cpp through tests/pair_option_main.cpp, plainly and under
-fsanitize=address,undefined."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import drop_pair_weights, pair_count, pair_fields, pair_index
from oracle.pyoracle import CpuModel, Csr
from util import STRESS_HP, rand_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ffm_engine_pair_ablation_enable", "ffm_engine_predict_pair_ablated", "ffm_engine_predict_pair_ablated_device",
                "ffm_engine_pair_ablation_read")
E_INVALID = fa.engine.E_INVALID


def test_numbering_round_trip_for_every_field_count():
    """pair_index(f, g) = f F - f (f - 1) / 2 + (g - f) for f <= g numbers the upper triangle row by row:
    numpy.triu_indices is the same order.  Both orders of (f, g); pair_fields is the inverse; pair_count = V."""
    for F in range(1, 65):
        fs, gs = np.triu_indices(F)
        V = F * (F + 1) // 2
        assert pair_count(F) == V == fs.size
        for v, (f, g) in enumerate(zip(fs.tolist(), gs.tolist())):
            assert f * F - f * (f - 1) // 2 + (g - f) == v
            assert pair_index(F, f, g) == v and pair_index(F, g, f) == v, (F, f, g)
            assert pair_fields(F, v) == (f, g), (F, v)
    assert pair_count(39) == 780 and pair_count(64) == 2080


def test_numbering_refusals():
    for call in (lambda: pair_count(0), lambda: pair_count(65), lambda: pair_index(65, 0, 0), lambda: pair_index(6, 6, 0),
                 lambda: pair_index(6, 0, -1), lambda: pair_fields(6, 21), lambda: pair_fields(6, -1), lambda: pair_fields(0, 0)):
        with pytest.raises(fa.EngineError) as ei:
            call()
        assert ei.value.code == E_INVALID
    assert "the row itself" in str(pytest.raises(fa.EngineError, pair_fields, 6, 21).value)


def three_field_block():
    """3 fields, ids 4 f .. 4 f + 3 under field f only.  Rows: all three fields with two entries of field 1; fields
    0 and 2 only; field 1 only, twice; fields 0 and 1; empty."""
    rows = [[(0, 0), (1, 4), (2, 8), (1, 5)], [(0, 1), (2, 9)], [(1, 6), (1, 7)], [(0, 2), (1, 4)], []]
    field = np.array([f for r in rows for f, _ in r], np.int32)
    feat = np.array([i for r in rows for _, i in r], np.int32)
    val = np.array([1.0, 0.5, 1.25, 1.0, 0.75, 1.0, 1.0, 0.3, 1.0, 2.0], np.float32)
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return Csr(row_ptr, field, feat, val, np.array([1, 0, 1, 0, 0], np.int32))


def test_zeroed_slot_is_the_pair_left_out_on_the_oracle():
    """The yardstick, not the kernel: CpuModel.predict_batch with slot (f, g) zeroed equals the whole row bit for
    bit on rows that lack f or g (f == g: that have fewer than two entries of f) and differs on a row that has
    both; and it equals the sum written out in Python with the pair's terms left out."""
    F, k, per = 3, 4, 4
    blk = three_field_block()
    assert np.array_equal(blk.field, blk.feat // per), "every id under one field only"
    o = CpuModel("oracle", "FFM", F * per, F, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(11), o)
    assert st["bias3"][:1].view(np.uint32)[0] != 0x80000000, "the bias is not -0.0"
    o.set_state(st)
    whole, whole_loss = o.predict_batch(blk)
    w3 = st["vec_w"].reshape(F * per, F, k)
    counts = np.array([[int((blk.field[blk.row_ptr[r]:blk.row_ptr[r + 1]] == f).sum()) for f in range(F)] for r in range(blk.n_rows)])

    def by_hand(r, drop):
        """bias, linear products, then the pair terms in (a outer, b inner) order, fp32 throughout."""
        lo, hi = int(blk.row_ptr[r]), int(blk.row_ptr[r + 1])
        s = np.float32(st["bias3"][0])
        for p in range(lo, hi):
            s = np.float32(s + np.float32(st["lin_w"][blk.feat[p]] * blk.val[p]))
        for a in range(lo, hi):
            for b in range(a + 1, hi):
                fa_, fb_ = int(blk.field[a]), int(blk.field[b])
                if drop is not None and {fa_, fb_} == set(drop):
                    continue
                dot = np.float32(0.0)
                for j in range(k):
                    dot = np.float32(dot + np.float32(w3[blk.feat[a], fb_, j] * w3[blk.feat[b], fa_, j]))
                s = np.float32(s + np.float32(np.float32(dot * blk.val[a]) * blk.val[b]))
        return s

    for r in range(blk.n_rows):
        assert by_hand(r, None).view(np.uint32) == whole[r].view(np.uint32), r
    moved_somewhere = 0
    for f in range(F):
        for g in range(f, F):
            z = dict(st)
            z["vec_w"] = drop_pair_weights(w3, np.arange(f * per, (f + 1) * per), g).reshape(F * per, F * k)
            assert st["vec_w"].reshape(F * per, F, k)[f * per, g].any(), "drop_pair_weights returns a copy"
            oz = CpuModel("oracle", "FFM", F * per, F, k, **STRESS_HP)
            oz.set_state(z)
            got, got_loss = oz.predict_batch(blk)
            has_pair = (counts[:, f] >= 2) if f == g else ((counts[:, f] > 0) & (counts[:, g] > 0))
            assert np.array_equal(got[~has_pair].view(np.uint32), whole[~has_pair].view(np.uint32)), (f, g)
            assert (got[has_pair] != whole[has_pair]).all(), (f, g)
            for r in range(blk.n_rows):
                assert got[r].view(np.uint32) == by_hand(r, (f, g)).view(np.uint32), (f, g, r)
            if not has_pair.any():
                assert got_loss == whole_loss
            moved_somewhere += int(has_pair.any())
    assert moved_somewhere == 4  # (0, 1), (0, 2), (1, 1) and (1, 2) have rows; (0, 0) and (2, 2) have none
    assert counts[0].tolist() == [1, 2, 1] and counts[2].tolist() == [0, 2, 0]


def test_header_declares_the_entry_points_and_keeps_the_abi():
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    assert "#define FFM_ENGINE_ABI_VERSION 4" in header
    assert "Pair ablation" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(ffm_engine \*e," % name, code), name
    for name in ("ffm_engine_pair_count", "ffm_engine_pair_index", "ffm_engine_pair_fields"):
        assert re.search(r"\b%s\s*\(int32_t n_fields" % name, code), name
    for limit in ("n_fields > 64", "13 GB at 39 fields, 35 GB at 64", "FFM_E_NOMEM", "f * F - f * (f - 1) / 2 + (g - f)", "OUT OF SCOPE"):
        assert limit in header, limit


def test_library_exports_and_binding():
    fa.build()
    lib = fa.load_library()
    bound = {name: (res, args) for name, res, args in fa.ABI}
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and bound[name][0] is ctypes.c_int, name
    assert lib.ffm_engine_abi_version() == 4
    assert len(bound["ffm_engine_predict_pair_ablated"][1]) == len(bound["ffm_engine_predict_ablated"][1])
    assert len(bound["ffm_engine_predict_pair_ablated_device"][1]) == len(bound["ffm_engine_predict_ablated_device"][1])
    for fn, args in ((lib.ffm_engine_pair_ablation_enable, (None, 0)), (lib.ffm_engine_pair_ablation_read, (None, 0, None)),
                     (lib.ffm_engine_predict_pair_ablated, (None, 0, None, None, None, None, None, 0, None, None)),
                     (lib.ffm_engine_predict_pair_ablated_device, (None, 0, 0, None, None, None, None, None, 0, None, None))):
        assert fn(*args) == E_INVALID and b"null engine" in lib.ffm_engine_last_error()
    for name in ("pair_ablation_enable", "predict_pair_ablated", "predict_pair_ablated_device", "pair_ablation_metrics"):
        assert callable(getattr(fa.Engine, name))


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_cli_flag_refusals_and_lines(tmp_path, flags):
    """host/cmd_option.cpp and host/importance.cpp alone (tests/pair_option_main.cpp): the default, what is
    accepted, every refusal with its message, the numbering, the histogram memory, the printed lines of both flags."""
    exe = str(tmp_path / "pair_option")
    host = os.path.join(ROOT, "ftrl-ffm_amd", "host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", "pair_option_main.cpp"), os.path.join(host, "cmd_option.cpp"),
                         os.path.join(host, "importance.cpp"), "-ldl"], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    ffm = tmp_path / "d.ffm"
    ffm.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    svm = tmp_path / "d.svm"
    svm.write_text("1 1:1 7:0.5\n0 2:1 8:1\n")
    # the plain build also loads the engine library and compares its numbering (the kernel header's) with the host
    # copy's, pair by pair; the sanitized build stays what it is for: the new host code alone
    fa.build()
    more = [] if flags else [fa.LIB_PATH]
    out = subprocess.run([exe, str(ffm), str(svm), str(tmp_path / "lines.txt")] + more, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 22 + len(more), out.stdout
    assert ("the engine library numbers the pairs" in out.stdout) == bool(more)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_cli_refuses_before_a_device_is_opened(tmp_path):
    main_bin, _ = fa.build_host()
    ffm = tmp_path / "d.ffm"
    ffm.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    base = ["--model_type", "FFM", "--train_data", str(ffm), "--eval_data", str(ffm), "--pair_importance", "true"]
    for args, why in ((["--model_type", "FFM", "--train_data", str(ffm), "--pair_importance", "true"], "it needs --eval_data"),
                      (base + ["--n_fields", "65"], "--n_fields is 65, at most 64"),
                      (base + ["--n_factors", "12"], "--n_factors must be 4, 8, 16, 32 or 64 (got 12)")):
        out = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and out.stdout == "", (args, out.stdout)
        assert "invalid argument: --pair_importance true " in out.stderr and why in out.stderr, (args, out.stderr[:300])
        assert "--pair_importance <bool>" in out.stderr  # the help text follows
