"""GPU: ``train.py --method cps`` end to end on the synthetic scene -- the printed line, validation, checkpoints, exact
resume (eager and --graph), keep-best, ``predict.py`` on the result; ``trian_CPS.py`` is the same run."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--synthetic", "B2", "--synthetic_scene", "--num_unlabel", "700", "--print_per_batches", "3"]
LINE = re.compile(r"^Epoch (\d+)/3:  (\d+)/6 loss_contrast= (\d+\.\d\d) total_loss = (\d+\.\d{4}) cls_loss = (\d+\.\d{4}) "
                  r"con_loss = (\d+\.\d{4}) acc = (\d+\.\d\d)$")


def _py(script, *args, timeout=900):
    r = subprocess.run([sys.executable, script, *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _train(d, tag, *extra, script="train.py", method=("--method", "cps")):
    hist = os.path.join(d, f"hist_{tag}.npy")
    out = _py(script, *BASE, *method, "--num_epochs", "3", "--save_loss_hist", hist, *extra)
    return out, np.load(hist)


def _result_block(lines):
    i = lines.index("Result:")
    return [ln for ln in lines[i:] if not ln.startswith(("inference time ==", "validation check"))]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cps"))
    out, hist = _train(d, "S", "--eval_every", "1", "--save_eval", os.path.join(d, "S.npz"), "--ckpt_every", "1",
                       "--save_ckpt", os.path.join(d, "ck{epoch}.pt"), "--save_best", os.path.join(d, "best.pt"))
    return dict(dir=d, S=hist, S_out=out)


def test_the_run_prints_the_shared_line_and_learns(runs):
    out, hist = runs["S_out"], runs["S"]
    assert hist.shape == (18, 5) and np.isfinite(hist).all()
    assert (hist[:, 0] == hist[:, 3]).all()                                   # trian_CPS.py:254
    np.testing.assert_allclose(hist[:, 1], hist[:, 2] + 0.1 * hist[:, 3], rtol=1e-5)      # :245
    lines = [ln for ln in out if ln.startswith("Epoch ") and "loss_contrast" in ln]
    assert len(lines) == 6 and all(LINE.match(ln) for ln in lines), lines
    m = LINE.match(lines[0])
    assert m.group(3) == "%.2f" % np.mean(hist[:3, 0]) and m.group(6) == "%.4f" % np.mean(hist[:3, 3])
    assert sum(ln.startswith("Epoch ") and "validation" in ln for ln in out) == 6
    assert sum(ln.startswith(" OA") for ln in out) == 2 and sum(ln.startswith("AA") for ln in out) == 2
    # on the separable synthetic set the supervised loss of the last epoch is below the first's
    first, last = hist[:6, 2].mean(), hist[12:, 2].mean()
    print("cls_loss: first epoch %.4f, last epoch %.4f" % (first, last))
    assert last < first
    assert sorted(f for f in os.listdir(runs["dir"]) if f.endswith(".pt")) == ["best.pt", "ck1.pt", "ck2.pt", "ck3.pt"]


@pytest.mark.parametrize("mode", [(), ("--graph",)], ids=["eager", "graph"])
def test_resume_after_epoch_1_equals_the_straight_run_bit_for_bit(runs, mode):
    d, tag = runs["dir"], "R" + "".join(m.strip("-") for m in mode)
    out, hist = _train(d, tag, "--eval_every", "1", "--save_ckpt", os.path.join(d, tag + "_{epoch}.pt"),
                       "--resume", os.path.join(d, "ck1.pt"), *mode)
    assert hist.tobytes() == runs["S"].tobytes()                              # loss_hist
    assert _result_block(out) == _result_block(runs["S_out"])
    ep = [ln for ln in out if ln.startswith("Epoch ") and "loss_contrast" in ln]
    assert ep and all(ln.startswith(("Epoch 2/3", "Epoch 3/3")) for ln in ep)
    from cmlpl_amd import checkpoint
    a, b = checkpoint.load(os.path.join(d, "ck3.pt")), checkpoint.load(os.path.join(d, tag + "_3.pt"))
    for k in checkpoint.STATE_TENSORS:                                        # parameters, moments, (untouched) banks
        assert torch.equal(a[k], b[k]), k
    assert (a["ptr"], a["adam_t"], a["step_count"]) == (b["ptr"], b["adam_t"], b["step_count"]) == ([0, 0], 18, 18)
    assert a["identity"]["method"] == "cps" and a["identity"]["hp"]["w_mutual"] == pytest.approx(0.1)
    assert not a["bank_feats"].any()


def test_the_other_method_refuses_the_file_both_ways(runs, tmp_path):
    d = runs["dir"]
    r = subprocess.run([sys.executable, "train.py", *BASE, "--num_epochs", "3", "--no_eval", "--resume",
                        os.path.join(d, "ck1.pt")], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "--method cps" in r.stderr and "--method cmlpl" in r.stderr, r.stderr[-2000:]
    ck = str(tmp_path / "cmlpl.pt")
    _py("train.py", *BASE, "--num_epochs", "1", "--no_eval", "--save_ckpt", ck)
    from cmlpl_amd import checkpoint
    assert "method" not in checkpoint.load(ck)["identity"] and "method" not in checkpoint.load(ck)["extra"]["run"]
    r = subprocess.run([sys.executable, "train.py", *BASE, "--method", "cps", "--num_epochs", "3", "--no_eval", "--resume", ck],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "--method cps" in r.stderr and "--method cmlpl" in r.stderr, r.stderr[-2000:]


def test_predict_labels_the_scene_from_a_cps_checkpoint(runs):
    d = runs["dir"]
    labels = os.path.join(d, "labels.npy")
    out = _py("predict.py", "--ckpt", os.path.join(d, "ck3.pt"), "--synthetic", "B2", "--net", "both", "--out", labels)
    assert _result_block(out) == _result_block(runs["S_out"])                 # train.py's final labels, scored alike
    both = np.load(labels)
    assert both.shape == (2, 64 * 64) and both.dtype == np.int64
    _py("predict.py", "--ckpt", os.path.join(d, "best.pt"), "--synthetic", "B2", "--net", "0")


def test_trian_cps_is_the_same_run(runs):
    out, hist = _train(runs["dir"], "T", "--no_eval", script="trian_CPS.py", method=())
    assert hist.tobytes() == runs["S"].tobytes()


def test_cube_fed_cps_run_equals_the_split_fed_one(runs):
    out, hist = _train(runs["dir"], "C", "--no_eval", "--windows", "cube", "--graph")
    assert hist.tobytes() == runs["S"].tobytes()
