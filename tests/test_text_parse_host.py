"""The text grammar on the host (no GPU; include/ffm_engine.h "Text blocks", csrc/text_parse.h): the host twin
ffm_engine_textparse_host -- which the device kernels are pinned to in tests/test_gpu_text_parse.py -- against the
CLI's REAL parser, parse_csr_range of host/csr_reader.cpp (tests/text_parse_ref_main.cpp), bit for bit on texts made
of the grammar; every spelling outside it refused and reported; the twin once more as a stand-alone program under
-fsanitize=address,undefined (tests/text_parse_twin_main.cpp); and --device_parse as cmd_option.cpp parses it
(tests/device_parse_option_main.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import ftrl_ffm_amd as fa

import text_parse_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ftrl-ffm_amd", "host")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
KEYS = ("row_ptr", "label", "field", "feat", "val")


def _compile(tmp, name, main, sources, flags):
    exe = str(tmp / name)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fopenmp", "-pthread"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", main)] + [os.path.join(HOST, s) for s in sources] + ["-ldl"],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    return exe


def _read_dump(path):
    raw = open(path, "rb").read()
    head = np.frombuffer(raw[:48], np.int64)
    out = dict(zip(("n_lines", "n_rows", "nnz", "n_slow", "first_slow_byte", "overflow"), (int(x) for x in head)))
    body = np.frombuffer(raw[48:], np.int32)
    valid = out["n_rows"] >= 0 and out["n_slow"] == 0 and out["overflow"] == 0
    r, e = (out["n_rows"], out["nnz"]) if valid else (0, 0)
    sizes = [r + 1 if valid else 0, r, e, e, e]
    assert body.size == sum(sizes), (path, out, body.size)
    at = 0
    for k, n in zip(KEYS, sizes):
        out[k] = body[at:at + n]
        at += n
    out["val"] = out["val"].view(np.float32)
    return out


def _run_many(exe, head_args, texts, tmp, tag):
    """One process over all the texts: name -> dump."""
    args = []
    for name, text in texts.items():
        src, dst = tmp / ("%s_%s.txt" % (tag, name)), tmp / ("%s_%s.bin" % (tag, name))
        src.write_bytes(text)
        args += [str(src), str(dst)]
    out = subprocess.run([exe] + head_args + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    return {name: _read_dump(str(tmp / ("%s_%s.bin" % (tag, name)))) for name in texts}


def _same_block(a, b, what):
    assert a["n_rows"] == b["n_rows"] and a["nnz"] == b["nnz"], what
    for k in KEYS:
        x, y = a[k], b[k]
        if k == "val":
            x, y = x.view(np.uint32), y.view(np.uint32)  # the bits
        assert np.array_equal(x, y), (what, k)


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("ref"), "text_parse_ref", "text_parse_ref_main.cpp", ["csr_reader.cpp", "csr_stream.cpp"], [])


@pytest.mark.parametrize("has_field", [True, False], ids=["libffm", "libsvm"])
def test_twin_equals_the_real_parser_on_the_grammar(tmp_path, ref_exe, has_field):
    texts = cases.fast_texts(has_field)
    ref = _run_many(ref_exe, [str(int(has_field))], texts, tmp_path, "ref")
    for name, text in texts.items():
        twin = fa.parse_text_host(text, has_field=has_field)
        assert twin["n_slow"] == 0 and twin["overflow"] == 0 and twin["first_slow_byte"] == -1, name
        assert twin["n_lines"] == text.count(b"\n") + (0 if text.endswith(b"\n") or not text else 1), name
        assert ref[name]["n_rows"] >= 0, name
        _same_block(twin, ref[name], name)
        if not has_field:
            assert not twin["field"].any(), name
    # what the cases are there for
    z = fa.parse_text_host(texts["zeros"], has_field=has_field)
    assert z["n_rows"] == 2 and z["nnz"] == 1 and z["row_ptr"].tolist() == [0, 1, 1]
    lab = fa.parse_text_host(texts["labels"], has_field=has_field)
    assert lab["label"].tolist() == [1, 0, 0, 1, 1, 0, 0, 1, 1]
    lo = fa.parse_text_host(texts["label_only"], has_field=has_field)
    assert lo["n_rows"] == 6 and lo["nnz"] == 0 and lo["label"].tolist() == [1, 0, 0, 1, 1, 1]
    s = fa.parse_text_host(texts["signs"], has_field=has_field)
    assert s["val"].tolist() == [-1.5, 1.0, 0.5, -0.5, -7.0]
    assert fa.parse_text_host(texts["blank_lines"], has_field=has_field)["n_lines"] == 9
    assert fa.parse_text_host(texts["values"], has_field=has_field)["n_rows"] == 2000


@pytest.mark.parametrize("has_field", [True, False], ids=["libffm", "libsvm"])
def test_slow_spellings_are_refused_and_reported(tmp_path, ref_exe, has_field):
    slow = cases.slow_lines(has_field)
    texts, offsets = {}, {}
    for name, line in slow.items():
        texts[name], offsets[name] = cases.around(has_field, line)
    fast_only, _ = cases.around(has_field, "")
    fast_only = fast_only.replace(b"\n\n", b"\n")
    want = fa.parse_text_host(fast_only, has_field=has_field)
    assert want["n_rows"] == 3 and want["n_slow"] == 0
    ref = _run_many(ref_exe, [str(int(has_field))], texts, tmp_path, "slow")
    for name, text in texts.items():
        twin = fa.parse_text_host(text, has_field=has_field)
        assert twin["n_slow"] == 1 and twin["first_slow_byte"] == offsets[name], (name, twin)
        assert twin["n_lines"] == 4 and twin["n_rows"] == 3 and twin["overflow"] == 0, (name, twin)
        assert twin["row_ptr"].size == 0 and twin["val"].size == 0, name
        r = ref[name]
        if name in cases.MALFORMED:
            assert r["n_rows"] == -1, name  # `wrong input:`, with and without the device parser
            continue
        # the real parser takes the line, and what it makes of the lines around it is what the twin makes of them:
        # a chunk that falls back whole loses nothing and changes nothing
        assert r["n_rows"] == 4, (name, r["n_rows"])
        b, e = int(r["row_ptr"][2]), int(r["row_ptr"][3])
        rest = dict(n_rows=3, nnz=r["nnz"] - (e - b), label=np.delete(r["label"], 2),
                    row_ptr=np.concatenate([r["row_ptr"][:3], r["row_ptr"][3:][1:] - (e - b)]))
        for k in ("field", "feat", "val"):
            rest[k] = np.delete(r[k], np.arange(b, e))
        _same_block(want, rest, name)
    # a line of exactly FFM_TEXT_MAX_LINE bytes is not slow
    edge, _ = cases.around(has_field, slow["long_line"][:fa.TEXT_MAX_LINE])
    assert fa.parse_text_host(edge, has_field=has_field)["n_slow"] == 0
    # two slow lines: both counted, the earlier one reported
    two = texts["exponent"] + texts["nan"]
    twin = fa.parse_text_host(two, has_field=has_field)
    assert twin["n_slow"] == 2 and twin["first_slow_byte"] == offsets["exponent"] and twin["n_rows"] == 6


def test_capacities_and_arguments():
    text = cases.fast_texts(True)["synth"]
    full = fa.parse_text_host(text)
    R, E = full["n_rows"], full["nnz"]
    assert (R, E) == (300, 2400)
    exact = fa.parse_text_host(text, max_rows=R, max_nnz=E)
    _same_block(exact, full, "exact capacities")
    for kw in (dict(max_rows=R - 1, max_nnz=E), dict(max_rows=R, max_nnz=E - 1), dict(max_rows=0, max_nnz=0)):
        over = fa.parse_text_host(text, **kw)
        assert over["overflow"] == 1 and (over["n_rows"], over["nnz"], over["n_lines"]) == (R, E, R), kw
        assert over["row_ptr"].size == 0
    empty = fa.parse_text_host(b"")
    assert (empty["n_lines"], empty["n_rows"], empty["nnz"]) == (0, 0, 0) and empty["row_ptr"].tolist() == [0]
    assert fa.parse_text_host(b"\n")["n_lines"] == 1 and fa.parse_text_host(b"1")["label"].tolist() == [1]
    lib = fa.load_library()
    assert lib.ffm_engine_textparse_host(1, None, 4, 1, 1, None, None, None, None, None, None) == -1
    with pytest.raises(fa.EngineError):
        fa.parse_text_host(b"1\n", max_rows=-1)


def test_binding_constants_are_the_kernels_own():
    src = open(os.path.join(ROOT, "ftrl-ffm_amd", "csrc", "kernels_text.h")).read()
    for name, value in (("kTextTileBytes", fa.TEXT_TILE_BYTES), ("kTextScanBytes", fa.TEXT_SCAN_BYTES),
                        ("kTextLineTile", fa.TEXT_LINE_TILE), ("kTextScanChunk", fa.TEXT_SCAN_CHUNK)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == value, name
    grammar = open(os.path.join(ROOT, "ftrl-ffm_amd", "csrc", "text_parse.h")).read()
    assert int(re.search(r"kMaxLine = (\d+);", grammar).group(1)) == fa.TEXT_MAX_LINE
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    assert int(re.search(r"#define FFM_TEXT_MAX_LINE (\d+)", header).group(1)) == fa.TEXT_MAX_LINE


def test_twin_standalone_under_sanitizers(tmp_path):
    """The twin alone, with its own main and nothing preloaded, under ASan + UBSan over every text above, the slow
    ones included; its arrays have exactly the capacities it is given, here the block's own sizes and one less."""
    exe = _compile(tmp_path, "text_parse_twin", "text_parse_twin_main.cpp", [], SAN)
    for has_field in (True, False):
        texts = dict(cases.fast_texts(has_field))
        for name, line in cases.slow_lines(has_field).items():
            texts["slow_" + name] = cases.around(has_field, line)[0]
        texts["empty"] = b""
        tag = "ffm" if has_field else "svm"
        got = _run_many(exe, [str(int(has_field)), "-1", "-1"], texts, tmp_path, tag)
        for name, text in texts.items():
            want = fa.parse_text_host(text, has_field=has_field)
            for k in ("n_lines", "n_rows", "nnz", "n_slow", "first_slow_byte", "overflow"):
                assert got[name][k] == want[k], (name, k)
            _same_block(got[name], want, name)
        one = {"synth": texts["synth"]}
        full = fa.parse_text_host(texts["synth"], has_field=has_field)
        tight = _run_many(exe, [str(int(has_field)), str(full["n_rows"]), str(full["nnz"])], one, tmp_path, tag + "_tight")
        _same_block(tight["synth"], full, "tight")
        over = _run_many(exe, [str(int(has_field)), str(full["n_rows"] - 1), str(full["nnz"] - 1)], one, tmp_path, tag + "_over")
        assert over["synth"]["overflow"] == 1 and over["synth"]["n_rows"] == full["n_rows"] and over["synth"]["nnz"] == full["nnz"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_cli_option(tmp_path, flags):
    """--device_parse parsed by cmd_option.cpp alone (tests/device_parse_option_main.cpp): the default, what is
    accepted, and the two refusals with no device."""
    exe = _compile(tmp_path, "device_parse_option", "device_parse_option_main.cpp", ["cmd_option.cpp"], flags)
    data = tmp_path / "d.ffm"
    data.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    assert out.stdout.count("ok  ") == 9, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
