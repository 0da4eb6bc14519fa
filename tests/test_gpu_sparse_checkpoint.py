"""Sparse resumable checkpoints: Engine.sparse_state / load_sparse_state restore a model bit for bit into a
fresh engine of the same seed, and the CLI's --checkpoint_path / --resume_from make an interrupted and
resumed run THE uninterrupted run (same model files byte for byte, same printed losses)."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from scan_util import without_fields
from util import DEFAULT_HP, GOLDEN, STRESS_HP, assert_bitwise, assert_state_bitwise

pytestmark = pytest.mark.gpu

F, NF = 8, 5000


def make_engine(mt, k, learn, hp, seed=42):
    nfl = F if mt == "FFM" else 1
    fs = (np.arange(F + 1) * (NF // F)).astype(np.int32) if mt == "FFM" else None
    return fa.Engine(mt, NF, nfl, k, seed=seed, max_batch_rows=512, max_batch_nnz=512 * F, field_start=fs,
                     learn=learn, **hp)


@pytest.mark.parametrize("mt,k,learn,hp", [("FFM", 4, False, DEFAULT_HP), ("FFM", 4, True, STRESS_HP),
                                           ("FFM", 3, False, STRESS_HP), ("FM", 16, False, DEFAULT_HP),
                                           ("LR", 1, False, STRESS_HP)],
                         ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_restore_into_a_fresh_engine_is_bitwise(mt, k, learn, hp):
    gen = synth.Generator(F, NF, seed=9)
    blocks = [gen.block(512) for _ in range(4)]
    if mt != "FFM":
        blocks = [without_fields(b) for b in blocks]
    a = make_engine(mt, k, learn, hp)
    for b in blocks[:3]:
        a.train_batch(b)
    d = a.sparse_state()
    assert set(d) == {"ids", "bias3"} | set(fa.Engine.ROW_KEYS)
    n = d["ids"].size
    assert 0 < n < NF and (np.diff(d["ids"]) > 0).all()
    assert d["vec_w"].shape == (n, a.row_len) and d["lin_z"].shape == (n,)
    b_eng = make_engine(mt, k, learn, hp)
    b_eng.load_sparse_state(d)
    assert_state_bitwise(b_eng.get_state(), a.get_state(), "restored")
    la, sa = a.train_batch(blocks[3])
    lb, sb = b_eng.train_batch(blocks[3])
    assert_bitwise(lb, la, "logits of the fourth block")
    assert sa == sb or (np.isnan(sa) and np.isnan(sb))
    assert_state_bitwise(b_eng.get_state(), a.get_state(), "after the fourth block")
    # a model that has been touched is no base for deltas
    with pytest.raises(fa.EngineError) as err:
        b_eng.load_sparse_state(d)
    assert err.value.code == -1
    # ... nor is a fresh one of another seed the same base: the restored state then differs
    c = make_engine(mt, k, learn, hp, seed=43)
    c.load_sparse_state(d)
    if a.row_len:
        untouched = np.setdiff1d(np.arange(NF), d["ids"])[:8]
        assert (c.get_rows(untouched)["vec_w"] != a.get_rows(untouched)["vec_w"]).any()
    for e in (a, b_eng, c):
        e.close()


def _bundled(tmp_path):
    with gzip.open(os.path.join(GOLDEN, "data", "libffm_data.txt.gz"), "rt") as f:
        text = f.read()
    p = tmp_path / "libffm_data.txt"
    p.write_text(text)
    return str(p)


def _run(main_bin, tmp_path, args):
    out = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def _losses(stdout):
    return re.findall(r"epoch (\d+) train time: [0-9.]+s, train loss: ([0-9.]+)", stdout), \
        re.findall(r"epoch (\d+) eval time: [0-9.]+s, eval loss: ([0-9.]+)", stdout)


@pytest.mark.parametrize("online", ["true", "false"])
def test_cli_interrupted_and_resumed_run_is_the_uninterrupted_run(tmp_path, online):
    """FFM 8 x 16, 10 000 features on the bundled data: two epochs in one run against one epoch, a
    checkpoint, and one more epoch from it.  Online: the block-size ramp continues (rows_seen);
    offline: so does the shuffle sequence (seed + epoch number)."""
    main_bin, _ = fa.build_host()
    data = _bundled(tmp_path)
    base = ["--train_data", data, "--eval_data", data, "--model_type", "FFM", "--online", online,
            "--batch_size", "256"]
    out_a = _run(main_bin, tmp_path, base + ["--n_epochs", "2", "--model_path", "a.zst"])
    out_b1 = _run(main_bin, tmp_path, base + ["--n_epochs", "1", "--checkpoint_path", "c.ckpt"])
    out_b2 = _run(main_bin, tmp_path, base + ["--n_epochs", "1", "--resume_from", "c.ckpt", "--model_path", "b.zst"])
    for name in ("a.zst", "a.zst.nz"):
        a = (tmp_path / name).read_bytes()
        b = (tmp_path / name.replace("a.", "b.", 1)).read_bytes()
        assert len(a) > 1000 and a == b, name
    tr_a, ev_a = _losses(out_a)
    tr_1, ev_1 = _losses(out_b1)
    tr_2, ev_2 = _losses(out_b2)
    assert len(tr_a) == 2 and len(ev_a) == 2
    assert tr_1 == tr_a[:1] and ev_1 == ev_a[:1]
    assert tr_2 == tr_a[1:] and ev_2 == ev_a[1:]  # (epoch numbers included: the resumed run prints "epoch 2")
    # a checkpoint is a delta to ONE fresh model: another seed, another shape or a second load are refused
    for extra, msg in ((["--seed", "43"], "another seed"), (["--n_factors", "8"], "different shape"),
                       (["--init_stddev", "0.03"], "init parameters"), (["--learn", "true"], "--learn")):
        bad = subprocess.run([main_bin] + base + ["--n_epochs", "1", "--resume_from", "c.ckpt"] + extra, cwd=tmp_path,
                             capture_output=True, text=True, timeout=600)
        assert bad.returncode != 0 and msg in bad.stderr, bad.stderr


def test_cli_checkpoint_is_smaller_than_the_dense_pair(tmp_path):
    """200 000 features of which one 512-row Zipf block touches under 5 %: the checkpoint holds those
    records only, the dense pair all of them."""
    main_bin, _ = fa.build_host()
    nf, nfields, k = 200000, 8, 4
    blk = synth.Generator(nfields, nf, seed=3).block(512)
    touched = np.unique(blk.feat).size
    assert touched < 0.05 * nf
    data = tmp_path / "zipf.txt"
    data.write_text(synth.to_libffm_text(blk))
    out = _run(main_bin, tmp_path, ["--train_data", str(data), "--model_type", "FFM", "--n_feats", str(nf),
                                    "--n_fields", str(nfields), "--n_factors", str(k), "--n_epochs", "1",
                                    "--batch_size", "256", "--model_path", "d.zst", "--checkpoint_path", "d.ckpt"])
    ckpt = os.path.getsize(tmp_path / "d.ckpt")
    dense = os.path.getsize(tmp_path / "d.zst") + os.path.getsize(tmp_path / "d.zst.nz")
    print("checkpoint %d bytes, dense pair %d bytes, %d of %d features touched" % (ckpt, dense, touched, nf))
    assert ckpt < dense, (ckpt, dense, out)
    # the file says how many records it holds: exactly the ids of the block
    with open(tmp_path / "d.ckpt", "rb") as f:
        head = f.read(104)
    assert int.from_bytes(head[56:64], "little") == touched


def test_cli_sharded_models_refuse_checkpoints(tmp_path):
    """--n_gpus > 1 (the shards share the one device here): save_checkpoint and load_checkpoint throw."""
    main_bin, _ = fa.build_host()
    F_, per = 4, 100
    data = tmp_path / "s.ffm"
    data.write_text(synth.to_libffm_text(synth.Generator(F_, F_ * per, seed=5).block(64)))
    base = [main_bin, "--train_data", str(data), "--model_type", "FFM", "--n_fields", str(F_), "--n_feats", str(F_ * per),
            "--n_factors", "4", "--n_epochs", "1", "--batch_size", "64", "--field_ranges", "uniform"]
    ok = subprocess.run(base + ["--checkpoint_path", "one.ckpt"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert ok.returncode == 0, ok.stdout + ok.stderr
    env = dict(os.environ, FTRL_SAME_DEVICE="1")
    for extra in (["--checkpoint_path", "two.ckpt"], ["--resume_from", "one.ckpt"]):
        out = subprocess.run(base + ["--n_gpus", "2"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode != 0 and "not supported for sharded models" in out.stderr, out.stdout + out.stderr
    assert not (tmp_path / "two.ckpt").exists()
