"""The trainer CLI's --device_parse true on the bundled libffm data (10 000 rows, field 7 numeric): the three counting
passes -- --bucket_fields, --min_count, --field_ranges counted -- read the file as raw bytes and parse it on the
device, and write the same files and print the same summary lines as without the flag: one chunk, many chunks with
carried tails (FFM_TEXT_SLOT_BYTES), a value the device leaves to the host, a line longer than a slot, a malformed line.
(_bundled / run_cli are those of tests/test_gpu_scores_cli.py.)"""
import re
import subprocess

import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from test_gpu_scores_cli import _bundled, run_cli

pytestmark = pytest.mark.gpu

FLAGS = ["--model_type", "FFM", "--hash_feats", "true", "--bucket_fields", "7", "--min_count", "3", "--field_ranges", "counted",
         "--n_epochs", "0"]
OUTS = ("buckets", "rare", "ranges")
PARSE_LINE = re.compile(r"^device parse: (\d+) chunks, (\d+) bytes, (\d+) parsed by the host(?: \(first at byte (\d+)\))?\n", re.M)


def _args(path, tag):
    return FLAGS + ["--train_data", path, "--buckets_out", "buckets_%s.txt" % tag, "--rare_ids_out", "rare_%s.bin" % tag,
                    "--field_ranges_out", "ranges_%s.txt" % tag]


def _summary(stdout):
    """The passes' own lines, seconds masked; the device parser's lines are extra."""
    lines = [ln for ln in stdout.splitlines() if not ln.startswith("device parse:")]
    lines = [re.sub(r"_(host|dev)\.(txt|bin)", r"_X.\2", ln) for ln in lines]  # (the two runs' own file names)
    return [re.sub(r"in [0-9.]+ s", "in T s", re.sub(r"time: [0-9.]+s", "time: Ts", ln)) for ln in lines]


def _same_files(tmp_path, a, b):
    for k in OUTS:
        fa_, fb_ = (sorted(tmp_path.glob("%s_%s.*" % (k, t))) for t in (a, b))
        assert len(fa_) == 1 and len(fb_) == 1, k
        x, y = fa_[0].read_bytes(), fb_[0].read_bytes()
        assert len(x) > 0 and x == y, k


def _pair(tmp_path, path, tag, env=None):
    """The run without the flag and the run with it: (stdout, stdout)."""
    plain = run_cli(tmp_path, _args(path, tag + "_host"))
    dev = run_cli(tmp_path, _args(path, tag + "_dev") + ["--device_parse", "true"], env=env)
    _same_files(tmp_path, tag + "_host", tag + "_dev")
    assert _summary(plain) == _summary(dev)
    assert not PARSE_LINE.findall(plain)
    return plain, dev


def test_same_files_and_lines_one_chunk_and_many(tmp_path):
    path, text = _bundled(tmp_path)
    plain, dev = _pair(tmp_path, path, "one")
    assert any(ln.startswith("value buckets: counted 10000 rows") for ln in plain.splitlines())
    assert any(ln.startswith("rare ids: counted 10000 rows") for ln in plain.splitlines())
    assert sum(ln.startswith("field ranges: counted from 10000 rows") for ln in plain.splitlines()) == 1
    got = PARSE_LINE.findall(dev)
    assert got == [("1", str(len(text)), "0", "")] * 3, dev  # three passes, one chunk each, nothing left to the host
    # slots of 64 KB: 12 chunks or more, each cut at its last line end, the tail carried into the next
    _, dev = _pair(tmp_path, path, "many", env={"FFM_TEXT_SLOT_BYTES": "65536"})
    got = PARSE_LINE.findall(dev)
    assert len(got) == 3 and all(int(c) >= 12 and int(b) == len(text) and h == "0" for c, b, h, _ in got), dev
    _same_files(tmp_path, "one_dev", "many_dev")


def test_a_value_outside_the_grammar_goes_to_the_host(tmp_path):
    path, text = _bundled(tmp_path)
    lines = text.splitlines()
    assert lines[4321].split()[-1].startswith("7:")
    lines[4321] = " ".join(lines[4321].split()[:-1] + ["7:9803:1e-3"])
    lines[7000] = lines[7000] + " " * 70000  # longer than a 64 KB slot: the host parser's
    off = sum(len(ln) + 1 for ln in lines[:4321])
    p = tmp_path / "exp.txt"
    p.write_text("\n".join(lines) + "\n")
    n_bytes = p.stat().st_size
    _, dev = _pair(tmp_path, str(p), "exp")
    got = PARSE_LINE.findall(dev)
    assert got == [("1", str(n_bytes), "1", str(off))] * 3, dev
    _, dev = _pair(tmp_path, str(p), "expmany", env={"FFM_TEXT_SLOT_BYTES": "65536"})
    got = PARSE_LINE.findall(dev)
    assert len(got) == 3 and all(int(b) == n_bytes and h == "2" and int(first) == off for _, b, h, first in got), dev
    _same_files(tmp_path, "exp_dev", "expmany_dev")


def test_a_malformed_line_ends_the_run_the_same_way(tmp_path):
    path, text = _bundled(tmp_path)
    lines = text.splitlines()
    lines[2500] = "1 0:17:1 3:4: 5:6:1"
    p = tmp_path / "bad.txt"
    p.write_text("\n".join(lines) + "\n")
    main_bin, _ = fa.build_host()
    outs = []
    for extra in ([], ["--device_parse", "true"]):
        out = subprocess.run([main_bin] + _args(str(p), "bad") + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        outs.append(out)
        assert out.returncode != 0
        assert [ln for ln in out.stdout.splitlines() if ln.startswith("wrong input:")] == ["wrong input: " + lines[2500]], out.stdout
    assert outs[0].returncode == outs[1].returncode
    assert outs[0].stderr == outs[1].stderr
