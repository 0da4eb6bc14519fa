"""Rows without values, the part that needs no GPU: the facts the host mirror's readers note about a block
(tests/implicit_ones_main.cpp, plain and under -fsanitize=address,undefined), the synthetic generator's
opt-in switch, and the binding's handling of a block whose val is None."""
import os
import subprocess

import numpy as np
import pytest

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_block_facts_stand_alone(tmp_path, flags):
    """CsrBlock::push, CsrStream's token path, load_csr, slice, gather and a split block on hand-written rows:
    all ones, one -1.0f, one 1.0f + ulp, an empty block, rows out of field order, a row with a missing field, a
    multi-valued field."""
    host = os.path.join(ROOT, "ftrl-ffm_amd", "host")
    exe = str(tmp_path / "implicit_ones")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fopenmp", "-pthread"] + flags +
                        ["-o", exe, os.path.join(ROOT, "tests", "implicit_ones_main.cpp"),
                         os.path.join(host, "csr_reader.cpp"), os.path.join(host, "csr_stream.cpp")],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    work = tmp_path / "files"
    work.mkdir()
    out = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "FAIL" not in out.stdout, out.stdout
    for part in ("push: ", "stream: ", "load_csr + slice: ", "load_csr + gather: ", "split: "):
        assert part in out.stdout, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_synth_switch():
    """ones=None is the generator as it always was; "array" and "none" give the same ids with values of 1.0,
    spelled out or left away."""
    base = synth.Generator(6, 600, seed=3).block(50)
    again = synth.Generator(6, 600, seed=3, ones=None).block(50)
    for key in ("row_ptr", "field", "feat", "val", "label"):
        assert np.array_equal(getattr(base, key), getattr(again, key)), key
    assert (base.val.reshape(50, 6)[:, 5] != 1.0).any()
    arr = synth.Generator(6, 600, seed=3, ones="array").block(50)
    bare = synth.Generator(6, 600, seed=3, ones="none").block(50)
    assert arr.val.dtype == np.float32 and (arr.val.view(np.uint32) == 0x3f800000).all() and arr.val.size == 300
    assert bare.val is None and bare.nnz == 300
    for key in ("row_ptr", "field", "feat"):
        assert np.array_equal(getattr(arr, key), getattr(base, key)), key
        assert np.array_equal(getattr(bare, key), getattr(base, key)), key
    assert np.array_equal(arr.label, bare.label)
    part = bare.rows(10, 20)
    assert part.val is None and part.n_rows == 10 and np.array_equal(part.feat, base.feat[60:120])
    assert synth.to_libffm_text(bare) == synth.to_libffm_text(arr)
    with pytest.raises(ValueError):
        synth.Generator(6, 600, ones="yes")


def test_binding_passes_a_null_pointer_and_caches_it():
    """Engine._csr on a block with val=None: a NULL val argument, cached on the block like any other, and a
    fresh tuple once the block gets an array."""
    e = fa.Engine.__new__(fa.Engine)  # (no device: only the argument marshalling is looked at)
    e.model_type = fa.engine.FFM
    blk = synth.Generator(4, 400, seed=1, ones="none").block(8)
    args = e._csr(blk)
    assert args[0] == 8 and args[4] is None and args[2] is not None
    assert e._csr(blk) is args
    blk.field = None
    both = e._csr(blk)
    assert both is not args and both[2] is None and both[4] is None
    blk.val = np.ones(32, np.float32)
    assert e._csr(blk)[4] is not None
