"""GPU: ``train.py --ema --ensemble --tta`` together -- every validation curve, every ``Result:`` block and every late
checkpoint entry in one run, which no other test asks for at once -- and its ``--resume``.  The smallest synthetic shape
(W8), 2 epochs of 4 steps; two process starts."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["--synthetic", "W8", "--synthetic_scene", "--num_unlabel", "64", "--labeled_batch_size", "16", "--unlabeled_batch_size", "16",
       "--num_epochs", "2", "--ema", "--ensemble", "--tta", "--m", "2", "--eval_every", "1", "--ckpt_every", "1"]
VALIDATION = ["validation", "validation1", "validation_ens", "validation_ema", "validation_ema1"]      # per evaluation
RESULTS = ["OA", "OA1", "OA_ema", "OA_ema1", "OA_ens", "OA_tta"]
EXTRA = ["epoch", "num_batches", "loss_hist", "eval_epochs", "eval_curve", "eval_cms", "gen_state", "args", "run", "world",
         "eval_epochs_ema", "eval_curve_ema", "eval_cms_ema", "eval_epochs_ens", "eval_curve_ens", "eval_cms_ens"]
MEMBERS = ["curve", "epochs", "cm", "curve_ema", "cm_ema", "epochs_ema", "curve_ens", "cm_ens", "epochs_ens"]


def _train(d, tag, *extra):
    f = lambda name: os.path.join(d, tag + name)
    r = subprocess.run([sys.executable, "train.py", *RUN, "--save_loss_hist", f(".npy"), "--save_eval", f(".npz"),
                        "--save_ckpt", f("{epoch}.pt"), *extra], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _validation(lines):
    return [(int(m.group(1)), m.group(2)) for m in (re.match(r"Epoch (\d+)/2: (validation\w*) OA = ", ln) for ln in lines) if m]


def test_every_curve_at_once_and_its_resume(tmp_path):
    from cmlpl_amd import checkpoint
    d = str(tmp_path)
    S = _train(d, "S")
    R = _train(d, "R", "--resume", os.path.join(d, "S1.pt"))
    assert _validation(S) == [(epoch, name) for epoch in (1, 2) for name in VALIDATION]
    assert _validation(R) == [(2, name) for name in VALIDATION]
    for lines in (S, R):
        assert [m.group(1) for m in (re.match(r" (OA\w*)=", ln) for ln in lines) if m] == RESULTS
        assert [ln.split(":")[0] for ln in lines if ln.startswith("best validation")] == \
            ["best validation", "best validation1", "best validation_ens"]
    assert [ln for ln in R if "validation" in ln and "Epoch 2/2" in ln] == [ln for ln in S if "validation" in ln and "Epoch 2/2" in ln]
    hist_s, hist_r = np.load(os.path.join(d, "S.npy")), np.load(os.path.join(d, "R.npy"))
    assert hist_s.shape == (8, 5) and np.isfinite(hist_s).all() and hist_r.tobytes() == hist_s.tobytes()
    zs, zr = np.load(os.path.join(d, "S.npz")), np.load(os.path.join(d, "R.npz"))
    assert zs.files == MEMBERS and zr.files == MEMBERS
    for k in MEMBERS:
        assert zr[k].dtype == zs[k].dtype and zr[k].shape == zs[k].shape and zr[k].tobytes() == zs[k].tobytes(), k
    assert zs["curve"].shape == (2, 2, 3) and zs["curve_ema"].shape == (2, 2, 3) and zs["curve_ens"].shape == (2, 3)
    assert zs["cm"].shape == (2, 2, 5, 5) and zs["cm_ema"].shape == (2, 2, 5, 5) and zs["cm_ens"].shape == (2, 5, 5)
    assert all(zs["epochs" + sfx].tolist() == [1, 2] for sfx in ("", "_ema", "_ens"))
    first, a, b = (checkpoint.load(os.path.join(d, name)) for name in ("S1.pt", "S2.pt", "R2.pt"))
    for ck in (first, a, b):
        assert list(ck["extra"]) == EXTRA
    assert first["extra"]["eval_epochs_ens"] == [1] and tuple(first["extra"]["eval_curve_ema"].shape) == (1, 2, 3)
    assert set(a) == set(b)
    for k in checkpoint.STATE_TENSORS + ("teacher_params",):
        assert torch.equal(a[k], b[k]), k
    for key in ("Base", "Base1", "Teacher", "Teacher1"):
        assert list(a[key]) == list(b[key]) and all(torch.equal(a[key][k], b[key][k]) for k in a[key]), key
    for k in EXTRA:
        if isinstance(a["extra"][k], torch.Tensor):
            assert torch.equal(a["extra"][k], b["extra"][k]), k
        elif k != "args":                                           # (the two legs' file names differ)
            assert a["extra"][k] == b["extra"][k], k
