"""Pair masks without a device (include/ffm_engine.h "Pair masks"): the binding's pair_mask / pair_mask_pairs /
pair_mask_top, and host/pair_mask.{h,cpp} -- the mask file and the CLI's selection rule -- through the stand-alone
program tests/pair_mask_file_main.cpp, built with g++ once plain and once with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import pair_count, pair_fields, pair_index, pair_mask, pair_mask_pairs, pair_mask_top

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "pair_mask_file_main.cpp")
SRCS = [os.path.join(ROOT, "ftrl-ffm_amd", "host", "pair_mask.cpp")]


def test_the_new_symbols_are_declared_and_exported():
    lib = fa.load_library()
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    for name in ("ffm_engine_set_pair_mask", "ffm_engine_get_pair_mask"):
        assert "int %s(" % name in header and getattr(lib, name) is not None
    assert "pair masks or pruned tables" not in header and '"Pair masks" below' in header


@pytest.mark.parametrize("F", [1, 2, 6, 39, 64])
def test_pair_mask_and_pairs_are_inverses(F):
    rng = np.random.default_rng(F)
    every = [(f, g) for f in range(F) for g in range(f, F)]
    for density in (0.0, 0.3, 1.0):
        kept = [p for p in every if rng.random() < density or density == 1.0]
        words = pair_mask(F, [(g, f) if i % 2 else (f, g) for i, (f, g) in enumerate(kept)])  # (either order)
        assert words.dtype == np.uint64 and words.shape == (F,)
        assert pair_mask_pairs(words) == kept
        for f in range(F):
            assert F == 64 or int(words[f]) >> F == 0
            for g in range(F):
                assert (int(words[f]) >> g) & 1 == (int(words[g]) >> f) & 1 == ((min(f, g), max(f, g)) in set(kept))
        assert np.array_equal(pair_mask(F, pair_mask_pairs(words)), words)
    if F == 64:
        assert int(pair_mask(F, [(63, 63)])[63]) == 1 << 63 and int(pair_mask(F, [(0, 63)])[0]) == 1 << 63


def test_bad_fields_and_bad_words_are_refused():
    for bad in ((0, 6), (6, 0), (-1, 2), (2, -1)):
        with pytest.raises(ValueError):
            pair_mask(6, [bad])
    for F in (0, 65):
        with pytest.raises(ValueError):
            pair_mask(F, [])
    with pytest.raises(ValueError, match="symmetric"):
        pair_mask_pairs(np.array([2, 0, 0], np.uint64))
    with pytest.raises(ValueError, match="at or above"):
        pair_mask_pairs(np.array([8, 0, 0], np.uint64))
    with pytest.raises(ValueError):
        pair_mask_pairs(np.zeros(65, np.uint64))


def top_cases():
    """(n_fields, n_keep, loss[V + 1]) tables: distinct deltas, ties, negative deltas, N of 0 and V, non-finite."""
    rng = np.random.default_rng(11)
    cases = []
    for F in (1, 3, 6, 39, 64):
        V = pair_count(F)
        base = 100.0
        distinct = base + rng.permutation(V).astype(np.float64) - V / 3.0  # (a third of the deltas negative)
        tied = base + rng.integers(-2, 3, V).astype(np.float64)            # (five values: many ties, zeros among them)
        for loss in (distinct, tied):
            for n in sorted({0, 1, V // 4, V - 1 if V > 1 else 0, V}):
                cases.append((F, n, np.append(loss, base)))
    V = pair_count(3)
    for v, bad in ((0, np.nan), (4, np.inf), (5, -np.inf)):
        loss = np.append(np.arange(V, dtype=np.float64), 1.0)
        loss[v] = bad
        cases.append((3, 2, loss))
    cases.append((3, 2, np.append(np.arange(V, dtype=np.float64), np.nan)))  # (the rows' own loss)
    return cases


def test_pair_mask_top():
    F = 3  # pairs in index order: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    loss = np.array([5.0, 1.0, 3.0, 3.0, 0.0, 2.0, 1.0])  # deltas 4 0 2 2 -1 1
    want_order = [(0, 0), (0, 2), (1, 1), (2, 2), (0, 1), (1, 2)]  # largest first, the tie to the lower index, negative last
    for n in range(7):
        assert pair_mask_pairs(pair_mask_top(F, loss, n)) == sorted(want_order[:n]), n
    for bad_n in (-1, 7):
        with pytest.raises(ValueError):
            pair_mask_top(F, loss, bad_n)
    with pytest.raises(ValueError):
        pair_mask_top(F, loss[:-1], 2)
    for F, n, loss in top_cases():
        V = pair_count(F)
        if not np.isfinite(loss).all():
            with pytest.raises(ValueError, match=r"pair mask: loss without pair \d+ \d+ is not finite"):
                pair_mask_top(F, loss, n)
            continue
        kept = pair_mask_pairs(pair_mask_top(F, loss, n))
        assert len(kept) == n
        delta = loss[:V] - loss[V]
        kept_v = {pair_index(F, f, g) for f, g in kept}
        for v in kept_v:  # nothing left out beats, or ties with a lower index, something kept
            for u in set(range(V)) - kept_v if V <= 21 else ():
                assert delta[u] < delta[v] or (delta[u] == delta[v] and u > v), (F, n, u, v)
        if n and n < V:
            assert min(delta[v] for v in kept_v) >= max(delta[u] for u in set(range(V)) - kept_v)


def write_tables(path):
    with open(path, "w") as out:
        for F, n, loss in top_cases():
            out.write("%d %d\n" % (F, n))
            out.write(" ".join(repr(float(x)) for x in loss) + "\n")
            try:
                pairs = pair_mask_pairs(pair_mask_top(F, loss, n))
                out.write(" ".join("%d %d" % p for p in pairs) + "\n")
            except ValueError as e:
                out.write("refused %s\n" % e)
    return len(top_cases())


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_mask_file_and_selection_rule(tmp_path, flags):
    assert shutil.which("g++"), "g++ is needed to build the host code"
    exe = str(tmp_path / "pair_mask_file")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags + ["-o", exe, MAIN] + SRCS,
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    work = tmp_path / "files"
    work.mkdir()
    n_cases = write_tables(str(tmp_path / "tables"))
    out = subprocess.run([exe, str(work), str(tmp_path / "tables")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout, out.stdout
    assert out.stdout.count("round trip") == 9 and out.stdout.count("reject ") == 18 and out.stdout.count("selection ") == n_cases, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    # the file as the CLI writes it
    text = open(str(work / "mask_39_1")).read().split("\n")
    assert text[0] == "ffm-pair-mask 1 39 1" and len(text) == 3 and text[2] == ""
    f, g = (int(x) for x in text[1].split())
    assert (f, g) == pair_fields(39, pair_count(39) // 2)
