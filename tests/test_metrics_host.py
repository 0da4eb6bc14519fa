"""From a score histogram to AUC on the host (csrc/metrics_host.h behind
ffm_engine_metrics_from_histogram): exact integer arithmetic in a 128-bit accumulator, checked here
against Python integers and fractions.Fraction without a GPU, and as a stand-alone program
(tests/metrics_host_main.cpp) built with g++ alone, plainly and with -fsanitize=address,undefined."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ftrl_ffm_amd as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "metrics_host_main.cpp")


def exact(pos, neg):
    """(P, N, mixed bins, auc, slack) in Python integers; auc / slack are Fractions, None without pairs."""
    P = N = below = ties = mixed = 0
    pos, neg = np.asarray(pos, np.uint64), np.asarray(neg, np.uint64)
    filled = np.flatnonzero((pos != 0) | (neg != 0))  # (an empty bin adds nothing to any sum)
    for p, n in zip((int(v) for v in pos[filled]), (int(v) for v in neg[filled])):
        below += p * N
        ties += p * n
        mixed += 1 if p and n else 0
        P += p
        N += n
    if P * N == 0:
        return P, N, mixed, None, None
    return P, N, mixed, Fraction(2 * below + ties, 2 * P * N), Fraction(ties, 2 * P * N)


def ulps(got, want):
    """|got - want| in units of the spacing of doubles at `want` (a Fraction)."""
    if want == 0:
        return 0.0 if got == 0.0 else math.inf
    return float(abs(Fraction(got) - want) / Fraction(math.ulp(float(want))))


def check(pos, neg, n_nan=0):
    m = fa.metrics_from_histogram(pos, neg, n_nan)
    P, N, mixed, auc, slack = exact(pos, neg)
    assert (m["n_pos"], m["n_neg"], m["n_mixed_bins"], m["n_nan"]) == (P, N, mixed, n_nan)
    if auc is None:
        assert math.isnan(m["auc"]) and math.isnan(m["auc_slack"])
    else:
        # two integer -> double conversions and one divide, each within half an ulp
        assert ulps(m["auc"], auc) <= 4 and ulps(m["auc_slack"], slack) <= 4, (m, float(auc), float(slack))
        assert 0.0 <= m["auc"] <= 1.0 and 0.0 <= m["auc_slack"] <= 0.5
    return m


@pytest.mark.parametrize("n_bins", [1, 2, 7, 1 << 20])
def test_random_sparse_histograms_against_python_integers(n_bins):
    rng = np.random.default_rng(n_bins)
    for rep in range(4):
        pos = np.zeros(n_bins, np.uint64)
        neg = np.zeros(n_bins, np.uint64)
        filled = min(n_bins, 3000)
        cap = (9, 1000, 1 << 31, 1 << 40)[rep]
        pos[rng.integers(0, n_bins, filled)] = rng.integers(0, cap, filled).astype(np.uint64)
        neg[rng.integers(0, n_bins, filled)] = rng.integers(0, cap, filled).astype(np.uint64)
        if n_bins > 2:  # (the ends of the array count too)
            pos[-1] += 3
            neg[0] += 2
        check(pos, neg, n_nan=rep)


def test_all_ties_one_bin_holds_every_row():
    for n_bins in (1, 2, 7, 1 << 20):
        pos = np.zeros(n_bins, np.uint64)
        neg = np.zeros(n_bins, np.uint64)
        pos[n_bins // 2], neg[n_bins // 2] = 12, 30
        m = check(pos, neg)
        assert m["auc"] == 0.5 and m["auc_slack"] == 0.5 and m["n_mixed_bins"] == 1


def test_an_empty_class_gives_nan_and_still_succeeds():
    for n_bins in (1, 2, 7, 1 << 20):
        some = np.zeros(n_bins, np.uint64)
        some[n_bins - 1] = 4
        none = np.zeros(n_bins, np.uint64)
        m = check(some, none, n_nan=5)
        assert m["n_pos"] == 4 and m["n_neg"] == 0 and m["n_nan"] == 5 and math.isnan(m["auc"])
        m = check(none, some)
        assert m["n_neg"] == 4 and math.isnan(m["auc_slack"])
    m = check(np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    assert m["n_pos"] == 0 and math.isnan(m["auc"])


def test_counts_of_2_to_the_33_multiply_past_64_bits():
    c = 1 << 33
    m = check([c, c], [c, c])
    assert m["auc"] == 0.5 and m["auc_slack"] == 0.25 and m["n_pos"] == 2 * c
    m = check([0, c], [c, 3 * c])
    assert m["auc"] == 0.625 and m["auc_slack"] == 0.375
    big = np.zeros(1 << 20, np.uint64)
    big[[5, 1 << 19]] = c
    m = check(big, big[::-1].copy())
    assert m["n_pos"] == 2 * c and m["n_neg"] == 2 * c
    check([c + 1, c, 0, 3, c - 1, 0, 1], [c - 1, 0, c, c, 1, 2, c + 5])


def test_separated_classes_and_bad_arguments():
    assert check([0, 0, 5], [3, 1, 0])["auc"] == 1.0
    assert check([5, 0, 0], [0, 1, 3])["auc"] == 0.0
    with pytest.raises(ValueError):
        fa.metrics_from_histogram([1, 2], [1])
    lib = fa.load_library()
    assert lib.ffm_engine_metrics_from_histogram(None, None, 1, 0, None) == fa.engine.E_INVALID
    m = fa.Metrics()
    import ctypes
    assert lib.ffm_engine_metrics_from_histogram(None, None, 3, 0, ctypes.byref(m)) == fa.engine.E_INVALID
    assert b"null" in lib.ffm_engine_last_error()
    # without a device the engine's own calls refuse a null handle the usual way
    assert lib.ffm_engine_metrics_enable(None, 3) == fa.engine.E_INVALID
    assert lib.ffm_engine_metrics_read(None, 0, 0, ctypes.byref(m)) == fa.engine.E_INVALID
    assert lib.ffm_group_metrics_enable(None, 1) == fa.engine.E_INVALID


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_stand_alone_program_over_the_header(tmp_path, flags):
    assert shutil.which("g++"), "g++ is needed to build the host code"
    exe = str(tmp_path / "metrics_host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags + ["-o", exe, MAIN],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failed" in out.stdout and "FAILED" not in out.stdout, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
