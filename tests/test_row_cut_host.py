"""Where the blocks of --device_rows end, on the host (no GPU): the planner of host/row_cut.h -- which sees nothing of
a chunk but its row_ptr -- against CsrStream::next, the cut rule it restates (tests/row_cut_main.cpp: a stand-alone
program, run plainly and under -fsanitize=address,undefined), over texts with every row shape and chunk sizes under
which a block lies inside one chunk, spans two, spans three and more, and one chunk feeds several blocks; and
--device_rows as cmd_option.cpp parses it (tests/device_rows_option_main.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import row_cut_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ftrl-ffm_amd", "host")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
CASE = re.compile(r"^case (\d+) (\d+) (-?\d+): (\d+) blocks, (\d+) chunks, inside (\d+), two (\d+), three\+ (\d+), feeds (\d+)$")


def _compile(tmp, name, main, sources, flags):
    exe = str(tmp / name)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fopenmp", "-pthread"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", main)] + [os.path.join(HOST, s) for s in sources] + ["-ldl"],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    return exe


def _run(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "MISMATCH" not in out.stdout, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    return out.stdout.splitlines()


def test_the_texts_hold_every_row_shape():
    for seed, n_rows in ((0, 300), (1, 200), (2, 400)):
        text, counts = cases.make_text(n_rows, seed)
        assert 200 <= n_rows <= 400 and set(np.unique(counts)) == {0, 1, cases.N_FIELDS, 3 * cases.N_FIELDS}
        lines = text.split(b"\n")
        assert any(ln.strip(b"\r") in (b"0", b"1") for ln in lines), "a label-only line"
        assert any(ln and all(t.endswith(b":0") for t in ln.split()[1:]) and len(ln.split()) > 1 for ln in lines), "a row of zeros"
        assert b"\n\n" in text and b"\n   \n" in text and b"\r\n" in text and not text.endswith(b"\n")
    a = cases.chunks(text, 512)
    assert b"".join(a) == text and all(c.endswith(b"\n") for c in a[:-1]) and max(map(len, a)) <= 512 and len(a) > 10


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_planner_cuts_what_csr_stream_cuts(tmp_path, flags):
    exe = _compile(tmp_path, "row_cut", "row_cut_main.cpp", ["csr_reader.cpp", "csr_stream.cpp"], flags)
    seen = dict(inside=0, two=0, three=0, feeds=0)
    for seed, n_rows in ((0, 300), (1, 200), (2, 400)):
        text, counts = cases.make_text(n_rows, seed)
        path = tmp_path / ("t%d.ffm" % seed)
        path.write_bytes(text)
        budget = int(3 * counts.mean())  # an entry budget that bites: three mean rows
        assert budget >= counts.max(), "every single row fits"
        args = []
        for chunk_bytes in (256, 512, 4096, 1 << 20):
            for want in (1, 7, 64, 257, n_rows + 100):
                for max_nnz in (-1, budget):
                    args += [chunk_bytes, want, max_nnz]
        lines = _run(exe, [1, path] + args)
        assert len(lines) == len(args) // 3
        total_nnz = int(counts.sum())
        for line, i in zip(lines, range(0, len(args), 3)):
            m = CASE.match(line)
            assert m, line
            chunk_bytes, want, max_nnz, blocks, n_chunks, inside, two, three, feeds = (int(x) for x in m.groups())
            assert (chunk_bytes, want, max_nnz) == tuple(args[i:i + 3])
            assert inside + two + three == blocks and n_chunks == len(cases.chunks(text, chunk_bytes))
            if max_nnz < 0:
                assert blocks == -(-n_rows // want), line
            else:  # the budget bites: more blocks than the rows alone would give, none over it
                assert blocks >= max(-(-n_rows // want), -(-total_nnz // max_nnz)), line
                if want >= 64:
                    assert blocks > -(-n_rows // want), line
            seen["inside"] += inside
            seen["two"] += two
            seen["three"] += three
            seen["feeds"] = max(seen["feeds"], feeds)
            if chunk_bytes == 256 and want >= 257 and max_nnz < 0:
                assert three >= 1, line  # a block of 257 rows spans many chunks of 256 bytes
            if chunk_bytes == 4096 and want == 7 and max_nnz < 0:
                assert inside >= 1 and two >= 1 and feeds >= 2, line
    assert seen["inside"] and seen["two"] and seen["three"] and seen["feeds"] >= 2, seen


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_a_row_over_the_budget_is_refused_alike(tmp_path, flags):
    exe = _compile(tmp_path, "row_cut", "row_cut_main.cpp", ["csr_reader.cpp", "csr_stream.cpp"], flags)
    text, counts = cases.make_text(300, 0)
    path = tmp_path / "t.ffm"
    path.write_bytes(text)
    over = int(counts.max()) - 1  # the longest rows do not fit
    lines = _run(exe, [1, path, 512, 64, over, 256, 1, over, 1 << 20, 500, 2])
    assert len(lines) == 3
    for line in lines:
        assert line.endswith("length_error a row has more entries than a block can hold (max_nnz)"), line
    # libsvm text through the same planner
    text, counts = cases.make_text(250, 3, has_field=False)
    path = tmp_path / "t.svm"
    path.write_bytes(text)
    lines = _run(exe, [0, path, 300, 7, -1, 300, 64, int(3 * counts.mean())])
    assert all(CASE.match(line) for line in lines) and len(lines) == 2, lines


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_cli_option(tmp_path, flags):
    """--device_rows parsed by cmd_option.cpp alone (tests/device_rows_option_main.cpp): the default, what is accepted,
    and each refusal with no device."""
    exe = _compile(tmp_path, "device_rows_option", "device_rows_option_main.cpp", ["cmd_option.cpp"], flags)
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 18, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_reference_blocks_helper_is_the_cut_rule():
    """tests/row_cut_cases.reference_blocks (what the GPU tests slice host arrays by) on a hand-made row_ptr."""
    rp = [0, 2, 2, 7, 8, 20, 21]
    assert cases.reference_blocks(rp, [2], 1 << 30) == [(0, 2), (2, 4), (4, 6)]
    assert cases.reference_blocks(rp, [1, 2, 64], 1 << 30) == [(0, 1), (1, 3), (3, 6)]
    assert cases.reference_blocks(rp, [64], 8) == [(0, 4), (4, 5), (5, 6)]  # (the row of 12 goes out alone)
