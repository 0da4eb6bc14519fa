"""The trainer CLI's --serve_weights f8: a checkpoint scored by `--resume_from ck --n_epochs 0 --serve_weights f8
--predict_data F --predict_out P` gives, line by line, what the binding's f8 serving engine predicts after loading the
same trained model, and prints the format's two lines.  (The helpers are tests/test_gpu_scores_cli.py's.)"""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from test_gpu_scores_cli import BATCH, _bundled, parse_libffm, read_scores, run_cli, train_online
from util import assert_bitwise

pytestmark = pytest.mark.gpu
NF, F, K = 10000, 8, 16  # the CLI's defaults
BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH), "--learn", "true"]


def test_scoring_a_checkpoint_from_an_f8_serving_engine(tmp_path):
    path, text = _bundled(tmp_path)
    data = parse_libffm(text)
    n = data.n_rows
    run_cli(tmp_path, BASE + ["--train_data", path, "--n_epochs", "1", "--checkpoint_path", "ck"])
    out = run_cli(tmp_path, BASE + ["--resume_from", "ck", "--n_epochs", "0", "--serve_weights", "f8", "--predict_data", path,
                                    "--predict_out", "p.txt"])
    assert ("serving weights: f8, %d bytes of model\n" % (4 + 4 * NF + NF * fa.serve_f8_stride(F * K))) in out, out
    t = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, learn=True)
    train_online(t, data, BATCH, fa.default_batch_ramp(1e-4), 1)
    s = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, learn=True, serve="f8")
    sp = t.sparse_state()
    s.load_sparse_weights(sp)
    want = np.concatenate([s.predict_batch(data.rows(p, min(n, p + BATCH)), output_prob=True)[0] for p in range(0, n, BATCH)])
    assert_bitwise(read_scores(tmp_path / "p.txt")[0], want, "CLI --serve_weights f8 against the binding's f8 serving engine")
    st = s.encode_stats()
    line = "f8 pack: n_latent %d, n_inexact %d, n_to_inf %d, n_to_zero %d\n" % tuple(st[key] for key in ("n_latent", "n_inexact", "n_to_inf", "n_to_zero"))
    assert st["n_latent"] == sp["ids"].size * F * K and st["n_inexact"] > 0 and line in out, out
    t.close()
    s.close()
