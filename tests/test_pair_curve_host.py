"""The pruning curve, the part that needs no GPU (include/ffm_engine.h "Pruning curve"): pair_curve_levels and
pair_curve_mask against a direct double loop; the header declares the entry points, the library exports them and the
binding has the methods; the CLI flags --pair_curve / --pair_loss_budget, their refusals, the old --pair_keep /
--pair_mask_out refusals and the host's ranking, level table, budget pick and lines through
tests/pair_curve_option_main.cpp, plainly and under -fsanitize=address,undefined."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import pair_count, pair_curve_levels, pair_curve_mask, pair_fields, pair_index, pair_mask, pair_mask_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ffm_engine_pair_curve_enable", "ffm_engine_predict_pair_curve", "ffm_engine_predict_pair_curve_device",
                "ffm_engine_pair_curve_read")
FIELD_COUNTS = (1, 2, 6, 39, 64)


def auto_list(V):
    """round(i V / 63) for i = 0 .. 63, deduplicated (i V / 63 is never half an integer: 2 i V is even, 63 odd)."""
    out = []
    for i in range(64):
        n = (2 * i * V + 63) // 126
        assert abs(n - i * V / 63.0) < 0.5
        if not out or out[-1] != n:
            out.append(n)
    return out


@pytest.mark.parametrize("F", FIELD_COUNTS)
def test_levels_and_masks_against_a_double_loop(F):
    V = pair_count(F)
    order = np.random.default_rng(F).permutation(V)
    level = pair_curve_levels(F, order)
    assert level.dtype == np.uint16 and level.shape == (F, F) and np.array_equal(level, level.T)
    for f in range(F):
        for g in range(F):
            v = pair_index(F, f, g)
            assert order[level[f, g]] == v, (F, f, g)
    assert sorted(level[np.triu_indices(F)].tolist()) == list(range(V))
    cuts = sorted({0, 1, V // 3, V - 1, V, 65536} | set(auto_list(V)[::7]))
    for cut in cuts:
        words = pair_curve_mask(level, cut)
        assert words.dtype == np.uint64 and words.shape == (F,)
        want = [0] * F
        for f in range(F):
            for g in range(F):
                if int(level[f, g]) < cut:
                    want[f] |= 1 << g
        assert [int(w) for w in words] == want, (F, cut)
        # the round trip: the kept pairs are the first `cut` of the order, and pair_mask makes the same words of them
        kept = pair_mask_pairs(words)
        assert kept == sorted(pair_fields(F, int(v)) for v in order[:min(cut, V)]), (F, cut)
        assert np.array_equal(pair_mask(F, kept), words)
    assert not pair_curve_mask(level, 0).any() and len(pair_mask_pairs(pair_curve_mask(level, V))) == V
    # levels that are no ranks: duplicates and 65535
    rng = np.random.default_rng(100 + F)
    a = rng.integers(0, 4, (F, F)) * 21845
    free = (np.triu(a) + np.triu(a, 1).T).astype(np.uint16)
    for cut in (0, 1, 21845, 21846, 65535, 65536):
        words = pair_curve_mask(free, cut)
        for f in range(F):
            for g in range(F):
                assert ((int(words[f]) >> g) & 1) == int(int(free[f, g]) < cut), (F, cut, f, g)
    assert len(pair_mask_pairs(pair_curve_mask(free, 65536))) == V


def test_helpers_refuse_what_is_no_table_or_order():
    with pytest.raises(ValueError):
        pair_curve_levels(6, np.arange(20))
    with pytest.raises(ValueError):
        pair_curve_levels(6, np.zeros(21, np.int64))
    with pytest.raises(ValueError):
        pair_curve_levels(65, np.arange(65 * 33))
    level = pair_curve_levels(6, np.arange(21))
    lopsided = level.copy()
    lopsided[1, 4] += 1
    for bad, cut in ((lopsided, 3), (level[:5], 3), (level, -1), (level, 65537), (level.astype(np.float32), 3)):
        with pytest.raises(ValueError):
            pair_curve_mask(bad, cut)


def test_auto_list_values():
    for V, n in ((21, 22), (780, 64), (2080, 64)):
        a = auto_list(V)
        assert len(a) == n and a[0] == 0 and a[-1] == V and a == sorted(set(a))
        assert a == sorted({int(np.floor(i * V / 63.0 + 0.5)) for i in range(64)})
    assert auto_list(780)[:4] == [0, 12, 25, 37] and auto_list(2080)[1] == 33


def test_entry_points_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    fa.build()
    lib = ctypes.CDLL(fa.LIB_PATH)
    for name in ENTRY_POINTS:
        assert ("int %s(" % name) in header, name
        assert getattr(lib, name) is not None
    assert "Pruning curve" in header
    for name in ("pair_curve_enable", "predict_pair_curve", "predict_pair_curve_device", "pair_curve_metrics"):
        assert callable(getattr(fa.Engine, name))


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_cli_flags_refusals_and_lines(tmp_path, flags):
    """host/cmd_option.cpp, host/pair_mask.cpp and host/importance.cpp alone (tests/pair_curve_option_main.cpp)."""
    exe = str(tmp_path / "pair_curve_option")
    host = os.path.join(ROOT, "ftrl-ffm_amd", "host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", "pair_curve_option_main.cpp"), os.path.join(host, "cmd_option.cpp"),
                         os.path.join(host, "pair_mask.cpp"), os.path.join(host, "importance.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    ffm = tmp_path / "d.ffm"
    ffm.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([exe, str(ffm), str(tmp_path / "lines.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") >= 41, out.stdout  # (the checks as first written; "0 failed" covers any added since)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_cli_refuses_before_a_device_is_opened(tmp_path):
    main_bin, _ = fa.build_host()
    ffm = tmp_path / "d.ffm"
    ffm.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    base = ["--model_type", "FFM", "--n_fields", "8", "--train_data", str(ffm), "--eval_data", str(ffm)]
    imp = base + ["--pair_importance", "true"]
    for args, why in ((base + ["--pair_curve", "0,5"], "it needs --pair_importance true"),
                      (imp + ["--pair_curve", "0,,5"], "--pair_curve takes auto or 1 to 64 comma-separated numbers of pairs"),
                      (imp + ["--pair_curve", ",".join(["1"] * 65)], "at most 64 numbers of pairs"),
                      (imp + ["--pair_curve", "0,37"], "37 is more than the 36 pairs"),
                      (imp + ["--pair_curve", "0,5", "--pair_loss_budget", "0.1", "--pair_keep", "5", "--pair_mask_out", "m.txt"], "not allowed together"),
                      (imp + ["--pair_loss_budget", "0.1", "--pair_mask_out", "m.txt"], "it needs --pair_curve"),
                      (imp + ["--pair_curve", "0,5", "--pair_loss_budget", "0.1"], "it needs --pair_mask_out")):
        out = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and out.stdout == "", (args, out.stdout)
        assert "invalid argument: " in out.stderr and why in out.stderr, (args, out.stderr[:300])
    assert not (tmp_path / "m.txt").exists()
