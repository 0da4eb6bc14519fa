"""Field ablation, the part that needs no GPU: drop_field (the definition, in numpy) against a per-row Python
loop; the oracle on a block with a field nobody holds removed; the header declares the four entry points and
keeps its ABI version, the library exports them; the CLI refuses --field_importance before a device is opened."""
import ctypes
import os
import re
import subprocess

import numpy as np

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import drop_field
from oracle.pyoracle import CpuModel, Csr
from util import ROW_FIELDS, ROW_IDS_PER_FIELD, STRESS_HP, rand_state, row_length_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ffm_engine_ablation_enable", "ffm_engine_predict_ablated", "ffm_engine_predict_ablated_device",
                "ffm_engine_ablation_read")


def drop_by_rows(blk, f):
    """The definition, row by row: every entry whose field is f goes, everything else stays in order."""
    row_ptr, field, feat, val = [0], [], [], []
    for r in range(blk.n_rows):
        for p in range(int(blk.row_ptr[r]), int(blk.row_ptr[r + 1])):
            if int(blk.field[p]) != f:
                field.append(int(blk.field[p]))
                feat.append(int(blk.feat[p]))
                val.append(blk.val[p])
        row_ptr.append(len(field))
    return (np.asarray(row_ptr, np.int32), np.asarray(field, np.int32), np.asarray(feat, np.int32), np.asarray(val, np.float32))


def ladder():
    blk, nf = row_length_block("FFM", ROW_FIELDS, ROW_IDS_PER_FIELD, 3)
    return blk, nf


def test_drop_field_against_a_per_row_loop():
    blk, _ = ladder()
    lens = np.diff(blk.row_ptr)
    counts = np.bincount(blk.field[(blk.field >= 0) & (blk.field < ROW_FIELDS)], minlength=ROW_FIELDS)
    assert (lens == 0).any() and counts.min() > blk.n_rows, "empty rows and multi-valued fields are among the cases"
    erased = (blk.field < 0) | (blk.field >= ROW_FIELDS) | (blk.feat < 0)
    assert erased.any()
    # every field of the model, a field no row holds (ROW_FIELDS + 7), the erased entries' own field numbers
    for f in list(range(ROW_FIELDS)) + [ROW_FIELDS + 7, ROW_FIELDS + 2, -1]:
        got = drop_field(blk, f)
        row_ptr, field, feat, val = drop_by_rows(blk, f)
        assert got.row_ptr.dtype == np.int32 and got.field.dtype == np.int32 and got.feat.dtype == np.int32
        assert np.array_equal(got.row_ptr, row_ptr) and np.array_equal(got.field, field), f
        assert np.array_equal(got.feat, feat) and np.array_equal(got.val.view(np.uint32), val.view(np.uint32)), f
        assert got.n_rows == blk.n_rows and np.array_equal(got.label, blk.label)
        assert not (got.field == f).any()
        if 0 <= f < ROW_FIELDS:  # erased entries of other fields are kept (the engine erases them, as always)
            assert int((erased & (blk.field != f)).sum()) == int(((got.field < 0) | (got.field >= ROW_FIELDS) | (got.feat < 0)).sum())
    none = drop_field(Csr(blk.row_ptr, blk.field, blk.feat, None, blk.label), 2)
    assert none.val is None and np.array_equal(none.feat, drop_field(blk, 2).feat)
    # an empty row stays an empty row; a row of one field alone becomes one
    one = Csr(np.array([0, 0, 3, 4], np.int32), np.array([1, 1, 1, 0], np.int32), np.array([5, 6, 7, 8], np.int32),
              np.ones(4, np.float32), np.array([0, 1, 0], np.int32))
    assert drop_field(one, 1).row_ptr.tolist() == [0, 0, 0, 1] and drop_field(one, 1).feat.tolist() == [8]


def test_oracle_without_a_field_nobody_holds():
    blk, nf = ladder()
    k = 8
    o = CpuModel("oracle", "FFM", nf, ROW_FIELDS, k, **STRESS_HP)
    o.set_state(rand_state(np.random.default_rng(5), o))
    for prob in (False, True):
        want, wl = o.predict_batch(blk, output_prob=prob)
        got, gl = o.predict_batch(drop_field(blk, ROW_FIELDS + 7), output_prob=prob)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and gl == wl
    # and a field that rows do hold moves the logits of exactly the rows that hold a surviving entry of it
    want = o.predict_batch(blk)[0]
    got = o.predict_batch(drop_field(blk, 0))[0]
    valid = (blk.feat >= 0) & (blk.feat < nf) & (blk.field == 0)
    row_of = np.repeat(np.arange(blk.n_rows), np.diff(blk.row_ptr))
    holds = np.zeros(blk.n_rows, bool)
    holds[row_of[valid]] = True
    assert np.array_equal(got[~holds].view(np.uint32), want[~holds].view(np.uint32))
    assert (got[holds] != want[holds]).any()


def test_header_declares_the_entry_points_and_keeps_the_abi():
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    assert "#define FFM_ENGINE_ABI_VERSION 4" in header
    assert "Field ablation" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(ffm_engine \*e," % name, code), name
    for limit in ("n_fields > 64", "{4, 8, 16, 32, 64}", "OUT OF SCOPE", "bit for bit"):
        assert limit in header, limit


def test_library_exports_and_binding():
    fa.build()
    lib = fa.load_library()
    bound = {name: (res, args) for name, res, args in fa.ABI}
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and bound[name][0] is ctypes.c_int, name
    assert lib.ffm_engine_abi_version() == 4
    assert len(bound["ffm_engine_predict_ablated"][1]) == len(bound["ffm_engine_predict_batch"][1])
    assert len(bound["ffm_engine_predict_ablated_device"][1]) == len(bound["ffm_engine_predict_batch_device"][1])
    for fn, args in ((lib.ffm_engine_ablation_enable, (None, 0)), (lib.ffm_engine_ablation_read, (None, 0, None)),
                     (lib.ffm_engine_predict_ablated, (None, 0, None, None, None, None, None, 0, None, None)),
                     (lib.ffm_engine_predict_ablated_device, (None, 0, 0, None, None, None, None, None, 0, None, None))):
        assert fn(*args) == fa.engine.E_INVALID and b"null engine" in lib.ffm_engine_last_error()
    for name in ("ablation_enable", "predict_ablated", "predict_ablated_device", "ablation_metrics"):
        assert callable(getattr(fa.Engine, name))


def test_cli_refuses_before_a_device_is_opened(tmp_path):
    main_bin, _ = fa.build_host()
    ffm = tmp_path / "d.ffm"
    ffm.write_text("1 0:1:1 1:7:0.5\n0 0:2:1 1:8:1\n")
    svm = tmp_path / "d.svm"
    svm.write_text("1 1:1 7:0.5\n0 2:1 8:1\n")
    base = ["--train_data", str(ffm), "--eval_data", str(ffm), "--field_importance", "true"]
    cases = [
        (["--model_type", "FFM", "--train_data", str(ffm), "--field_importance", "true"], "it needs --eval_data"),
        (["--model_type", "LR", "--train_data", str(svm), "--eval_data", str(svm), "--field_importance", "true"], "only FFM rows have"),
        (["--model_type", "FM", "--train_data", str(svm), "--eval_data", str(svm), "--field_importance", "true"], "only FFM rows have"),
        (["--model_type", "FFM", "--n_gpus", "2", "--field_ranges", "uniform"] + base, "--n_gpus > 1 is not allowed"),
        (["--model_type", "FFM", "--n_fields", "65"] + base, "--n_fields is 65, at most 64"),
        (["--model_type", "FFM", "--n_factors", "12"] + base, "--n_factors must be 4, 8, 16, 32 or 64 (got 12)"),
    ]
    for args, why in cases:
        out = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and out.stdout == "", (args, out.stdout)
        assert "invalid argument: --field_importance true " in out.stderr and why in out.stderr, (args, out.stderr[:300])
        assert "--field_importance <bool>" in out.stderr  # the help text follows
