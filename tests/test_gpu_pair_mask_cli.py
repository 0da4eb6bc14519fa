"""The trainer CLI's --pair_keep N --pair_mask_out FILE and --pair_mask @FILE on the synthetic 4-field file of
tests/test_gpu_pair_importance_cli.py: the mask file is what ftrl_ffm_amd.pair_mask_top makes of the loss sums the
binding's predict_pair_ablated gives on the same model and file; a run that loads the mask prints the eval loss and
writes the scores of the binding's masked predict_batch, from a training engine and from an fp16 serving engine; the
refusals exit before a device is opened.  (run_cli / parse_libffm / the schedule are those of
tests/test_gpu_scores_cli.py.)"""
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from test_gpu_pair_importance_cli import BASE, F, K, NF, ROWS, V
from test_gpu_scores_cli import BATCH, parse_libffm, read_scores, run_cli, train_online
from util import assert_bitwise

pytestmark = pytest.mark.gpu

KEEP = 4
KEPT_LINE = re.compile(r"^pair mask: kept (\d+) of (\d+) pairs, smallest kept delta ([-+]\d+\.\d+) -> (\S+)\n", re.M)
LOADED_LINE = re.compile(r"^pair mask: (\d+) of (\d+) pairs kept, from (\S+)\n", re.M)
EVAL_LINE = re.compile(r"^epoch 1 eval time: [0-9.]+s, eval loss: ([0-9.]+)\n", re.M)


def test_mask_written_then_served(tmp_path):
    text = synth.to_libffm_text(synth.Generator(F, NF, "zipf", seed=23).block(ROWS))
    path = tmp_path / "d.ffm"
    path.write_text(text)
    data = parse_libffm(text)
    n = data.n_rows
    run_cli(tmp_path, BASE + ["--train_data", str(path), "--n_epochs", "1", "--checkpoint_path", "ck"])
    # the same model through the binding: the pairs' loss sums, the file pair_mask_top predicts
    t = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, learn=True)
    train_online(t, data, BATCH, fa.default_batch_ramp(1e-4), 1)
    t.pair_ablation_enable()
    loss = np.zeros(V + 1)
    for p in range(0, n, BATCH):
        loss += t.predict_pair_ablated(data.rows(p, min(n, p + BATCH)), scores=False)[1]
    words = fa.pair_mask_top(F, loss, KEEP)
    kept = fa.pair_mask_pairs(words)
    assert len(kept) == KEEP and len({float(x) for x in loss[:V]}) > KEEP, "the ranking has something to decide"
    second = run_cli(tmp_path, BASE + ["--train_data", str(path), "--resume_from", "ck", "--n_epochs", "0", "--eval_data", str(path), "--pair_importance", "true",
                                       "--pair_keep", str(KEEP), "--pair_mask_out", "mask.txt"])
    assert (tmp_path / "mask.txt").read_text() == "ffm-pair-mask 1 %d %d\n" % (F, KEEP) + "".join("%d %d\n" % p for p in kept)
    smallest = min(loss[fa.pair_index(F, f, g)] - loss[V] for f, g in kept)
    assert KEPT_LINE.findall(second) == [(str(KEEP), str(V), "%+.6f" % (smallest / n), "mask.txt")], second
    assert second.index("pairs listed") < second.index("pair mask: kept")
    # the mask served: a training engine, and an fp16 serving engine filled from it
    s = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, learn=True, serve="f16")
    s.load_sparse_weights(t.sparse_state())
    served = BASE + ["--train_data", str(path), "--resume_from", "ck", "--n_epochs", "0", "--pair_mask", "@mask.txt", "--eval_data", str(path),
                     "--predict_data", str(path)]
    for fmt, e in (("none", t), ("f16", s)):
        unmasked = np.concatenate([e.predict_batch(data.rows(p, min(n, p + BATCH)), output_prob=True)[0] for p in range(0, n, BATCH)])
        e.set_pair_mask(words)
        blocks = [e.predict_batch(data.rows(p, min(n, p + BATCH)), output_prob=True) for p in range(0, n, BATCH)]
        want = np.concatenate([b[0] for b in blocks])
        assert (want.view(np.uint32) != unmasked.view(np.uint32)).any(), "the mask changes a score"
        out = run_cli(tmp_path, served + ["--predict_out", fmt + ".txt"] + ([] if fmt == "none" else ["--serve_weights", fmt]))
        assert LOADED_LINE.findall(out) == [(str(KEEP), str(V), "mask.txt")], out
        assert EVAL_LINE.findall(out) == ["%.4f" % (sum(b[1] for b in blocks) / n)], out
        assert out.index("pair mask:") < out.index("epoch 1 eval time")
        got, _ = read_scores(tmp_path / (fmt + ".txt"))
        assert_bitwise(got, want, "CLI --pair_mask scores, --serve_weights %s" % fmt)
        e.close()


def test_refusals_come_before_a_device_is_opened(tmp_path):
    text = synth.to_libffm_text(synth.Generator(F, NF, "zipf", seed=23).block(40))
    path = tmp_path / "d.ffm"
    path.write_text(text)
    (tmp_path / "mask.txt").write_text("ffm-pair-mask 1 %d 0\n" % F)
    main_bin, _ = fa.build_host()
    serve = BASE + ["--resume_from", "ck", "--n_epochs", "0", "--eval_data", str(path), "--pair_mask", "@mask.txt"]
    imp = BASE + ["--train_data", str(path), "--eval_data", str(path), "--n_epochs", "1"]

    def swap(args, flag, value):
        args = list(args)
        args[args.index(flag) + 1] = value
        return args

    cases = [
        (swap(serve, "--n_epochs", "1") + ["--train_data", str(path)], "--pair_mask"),
        (serve + ["--field_importance", "true"], "--field_importance"),
        (serve + ["--pair_importance", "true"], "--pair_importance"),
        (serve + ["--n_gpus", "2"], "--n_gpus"),
        (swap(serve, "--model_type", "FM"), "--pair_mask"),
        (swap(serve, "--model_type", "LR"), "--pair_mask"),
        (serve + ["--cmd", "true"], "--cmd"),
        (swap(serve, "--pair_mask", "mask.txt"), "--pair_mask"),
        (imp + ["--pair_importance", "true", "--pair_keep", "3"], "--pair_mask_out"),
        (imp + ["--pair_importance", "true", "--pair_mask_out", "m.txt"], "--pair_keep"),
        (imp + ["--pair_keep", "3", "--pair_mask_out", "m.txt"], "--pair_importance"),
        (imp + ["--pair_importance", "true", "--pair_keep", str(V + 1), "--pair_mask_out", "m.txt"], "--pair_keep"),
        (imp + ["--pair_importance", "true", "--pair_keep", "-1", "--pair_mask_out", "m.txt"], "--pair_keep"),
    ]
    for args, flag in cases:
        bad = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert bad.returncode != 0 and flag in bad.stderr.split("\n")[0], (args, bad.stderr[:300])
        assert bad.stdout == "", (args, bad.stdout)  # (refused before a device is opened: nothing is printed)
    assert not (tmp_path / "m.txt").exists()
