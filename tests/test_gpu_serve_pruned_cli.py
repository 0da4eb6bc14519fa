"""The trainer CLI's --serve_pruned true on the synthetic 4-field file of tests/test_gpu_pair_importance_cli.py: the run's
--predict_out and its evaluation lines are, byte for byte, those of the same command without the flag (the masked
unpruned serving engine), and the printed slot count and bytes are fa.pruned_layout's."""
import re

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from test_gpu_pair_importance_cli import BASE, F, K, NF, ROWS
from test_gpu_scores_cli import run_cli, without_times

pytestmark = pytest.mark.gpu

KEPT = [(0, 1), (0, 2), (2, 2)]  # field 3 keeps no partner: its features store nothing
TABLE_LINE = re.compile(r"^pruned serving table: (\d+) of (\d+) slots kept, (\d+) bytes of model\n", re.M)
HASHED = ["--hash_feats", "true", "--field_ranges", "uniform"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pruned_cli")
    (tmp / "d.ffm").write_text(synth.to_libffm_text(synth.Generator(F, NF, "zipf", seed=23).block(ROWS)))
    (tmp / "mask.txt").write_text("ffm-pair-mask 1 %d %d\n" % (F, len(KEPT)) + "".join("%d %d\n" % p for p in KEPT))
    run_cli(tmp, BASE + HASHED + ["--train_data", "d.ffm", "--n_epochs", "1", "--checkpoint_path", "ck"])
    return tmp


@pytest.mark.parametrize("fmt,extra", [("f32", []), ("f16", ["--device_rows", "true"])])
def test_the_pruned_run_is_the_masked_run(model, fmt, extra):
    served = BASE + HASHED + extra + ["--resume_from", "ck", "--n_epochs", "0", "--pair_mask", "@mask.txt", "--eval_data", "d.ffm",
                                      "--metrics", "auc", "--predict_data", "d.ffm", "--serve_weights", fmt]
    masked = run_cli(model, served + ["--predict_out", fmt + ".masked"])
    pruned = run_cli(model, served + ["--predict_out", fmt + ".pruned", "--serve_pruned", "true"])
    assert (model / (fmt + ".pruned")).read_bytes() == (model / (fmt + ".masked")).read_bytes()
    assert len((model / (fmt + ".pruned")).read_text().splitlines()) == ROWS
    lines = [[x for x in without_times(out).splitlines() if x.startswith("epoch ")] for out in (masked, pruned)]
    assert lines[0] == lines[1] and any("eval loss" in x for x in lines[0]) and any("auc" in x for x in lines[0]), pruned
    base, _ = fa.pruned_layout(fa.pair_mask(F, KEPT), np.arange(F + 1) * (NF // F))
    slots = int(base[-1])
    assert 0 < slots < NF * F
    assert TABLE_LINE.findall(pruned) == [(str(slots), str(NF * F), str(4 + 4 * NF + slots * K * {"f32": 4, "f16": 2}[fmt]))], pruned
    assert TABLE_LINE.findall(masked) == [] and "pair mask: %d of" % len(KEPT) in pruned
