"""The trainer CLI's --pair_curve LIST and --pair_loss_budget T --pair_mask_out FILE on the bundled libffm data: every
printed `keep N` loss is the evaluation loss a second run prints under --pair_mask @F', F' written by --pair_keep N on
the same model; the file written under the budget is the one --pair_keep N* writes, byte for byte; a budget no listed
N meets writes nothing and exits non-zero.  (run_cli and the bundled file are those of tests/test_gpu_scores_cli.py.)"""
import re
import subprocess

import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from test_gpu_scores_cli import BASE as PLAIN, _bundled, run_cli

pytestmark = pytest.mark.gpu

# (the learning variant and a step size at which one epoch moves the latent weights: with the defaults they stay where
# the L1 term holds them, every pair term is zero and the curve is flat)
BASE = PLAIN + ["--learn", "true", "--w_alpha", "0.05", "--w_l1", "0", "--w_l2", "0"]
F = 8                 # the CLI's default --n_fields, which the bundled file fits
V = F * (F + 1) // 2  # 36
LIST = [0, 5, V]
HEAD = re.compile(r"^pair curve: (\d+) rows, loss (\d+\.\d{6})(, auc \d+\.\d{6})?\n", re.M)
KEEP = re.compile(r"^keep (\d+) of (\d+) pairs: loss (\d+\.\d{6}) \(delta ([-+]\d+\.\d{6})\)(, auc \d+\.\d{6} \(delta [-+]\d+\.\d{6}\))?\n", re.M)
PICKED = re.compile(r"^pair mask: kept (\d+) of (\d+) pairs, loss delta ([-+]\d+\.\d{6}) within budget (-?\d+\.\d{6}) -> (\S+)\n", re.M)
EVAL_LINE = re.compile(r"^epoch 2 eval time: [0-9.]+s, eval loss: ([0-9.]+)\n", re.M)


def test_curve_lines_budget_and_mask_file(tmp_path):
    path, text = _bundled(tmp_path)
    n = len(text.splitlines())
    run_cli(tmp_path, BASE + ["--train_data", path, "--n_epochs", "2", "--checkpoint_path", "ck"])
    resumed = BASE + ["--train_data", path, "--resume_from", "ck", "--n_epochs", "0", "--eval_data", path, "--pair_importance", "true"]
    # ---- the curve alone, with the AUC parts
    first = run_cli(tmp_path, resumed + ["--pair_curve", ",".join(str(x) for x in LIST), "--metrics", "auc"])
    head, lines = HEAD.findall(first), KEEP.findall(first)
    assert len(head) == 1 and head[0][0] == str(n) and head[0][2], first
    assert [(int(a), int(b)) for a, b, *_ in lines] == [(x, V) for x in LIST] and all(l[4] for l in lines), first
    assert first.index("pairs listed") < first.index("pair curve:") < first.index("keep 0 of")
    assert lines[-1][2] == head[0][1] and float(lines[-1][3]) == 0.0, "keeping all V pairs is the rows' own loss"
    delta = {int(l[0]): float(l[3]) for l in lines}
    loss = {int(l[0]): float(l[2]) for l in lines}
    assert delta[0] != 0.0 and len(set(delta.values())) >= 2, "the pairs carry something on this model: %r" % (delta,)
    # ---- every point against a masked evaluation of the same N: --pair_keep N writes F', --pair_mask @F' evaluates
    for x in LIST:
        name = "keep%d.txt" % x
        run_cli(tmp_path, resumed + ["--pair_keep", str(x), "--pair_mask_out", name])
        masked = run_cli(tmp_path, BASE + ["--train_data", path, "--resume_from", "ck", "--n_epochs", "0", "--eval_data", path, "--pair_mask", "@" + name])
        got = EVAL_LINE.findall(masked)
        assert len(got) == 1, masked
        digits = len(got[0].split(".")[1])
        print("keep %d: curve loss %.6f, masked evaluation %s" % (x, loss[x], got[0]))
        # to the printed digits: the evaluation line has `digits` decimals, the curve's line six
        assert abs(loss[x] - float(got[0])) <= 0.5 * 10.0 ** -digits + 0.5e-6, (x, loss[x], got[0])
    # ---- a budget between two printed deltas: the smallest listed N at or under it
    ranked = sorted(set(delta.values()))
    budget = (ranked[0] + ranked[1]) / 2.0  # (the printed deltas are at least 1e-6 apart: no rounding decides the pick)
    chosen = min(x for x in LIST if delta[x] <= budget)
    assert any(delta[x] > budget for x in LIST if x < chosen) or chosen == LIST[0]
    assert any(delta[x] > budget for x in LIST), "the budget excludes something"
    second = run_cli(tmp_path, resumed + ["--pair_curve", ",".join(str(x) for x in reversed(LIST)), "--pair_loss_budget", repr(budget),
                                          "--pair_mask_out", "picked.txt"])
    assert [l[:4] for l in KEEP.findall(second)] == [l[:4] for l in lines] and not any(l[4] for l in KEEP.findall(second)), second
    assert PICKED.findall(second) == [(str(chosen), str(V), "%+.6f" % delta[chosen], "%.6f" % budget, "picked.txt")], second
    assert (tmp_path / "picked.txt").read_bytes() == (tmp_path / ("keep%d.txt" % chosen)).read_bytes()
    assert (tmp_path / "picked.txt").read_text().startswith("ffm-pair-mask 1 %d %d\n" % (F, chosen))
    # ---- no listed N meets the budget: nothing written, a line that says so, a non-zero exit
    main_bin, _ = fa.build_host()
    under = min(delta.values()) - 1.0
    bad = subprocess.run([main_bin] + resumed + ["--pair_curve", ",".join(str(x) for x in LIST), "--pair_loss_budget", repr(under), "--pair_mask_out", "none.txt"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and not (tmp_path / "none.txt").exists(), bad.stdout
    assert [l[:4] for l in KEEP.findall(bad.stdout)] == [l[:4] for l in lines], bad.stdout
    assert "pair mask: no listed number of pairs has a loss delta within budget" in bad.stdout and "nothing written" in bad.stdout
    assert "--pair_loss_budget" in bad.stderr
