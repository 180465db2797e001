"""GPU: per-epoch validation.  ``Evaluator`` through a ``TrainEngine`` after a few steps equals ``infer_cube`` +
``CalAccuracy`` on the same parameters (counts exact, metrics at 1e-12), ``tools.hyper_tools.test_acc`` takes an
``Evaluator``, and ``train.py --eval_every`` end to end: the printed curve, the check against the end-of-run evaluation,
and -- evaluation must not disturb training -- ``--save_loss_hist`` bit-equal to the same run without the option (eager,
``--graph``, ``--windows cube``); without the option the output is what it was."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12


def _trained_engine(shape, steps=3):
    from cmlpl_amd import HyperParams, NetShape, TrainEngine
    s = O.NetShape(*shape)
    bt = btu = 16
    eng = TrainEngine(NetShape(*shape), bt, btu, HyperParams(), device=DEV)
    eng.load_state_dict(0, O.closed_form_params(s, 1))
    eng.load_state_dict(1, O.closed_form_params(s, 2))
    d = lambda t: t.to(DEV)
    for i in range(steps):
        b = O.synthetic_batch(s, bt, btu, 500 + i)
        eng.step(d(b["XPl"]), d(b["Xl"]), d(b["Y"]), d(b["XPu"]), d(b["Xu"]), 1, i)
    return eng


@pytest.mark.parametrize("shape", [(103, 11, 11, 103, 9), (48, 15, 15, 48, 20)])
def test_evaluator_through_an_engine_equals_infer_cube_and_calaccuracy(shape, capsys):
    from cmlpl_amd import NetShape
    from cmlpl_amd.evaluate import Evaluator
    from cmlpl_amd.infer import infer_cube
    from cmlpl_amd.models import BaseNet2
    from tools.hyper_tools import CalAccuracy, test_acc
    C_, H, W, bands, K = shape
    rows, cols = 40, 36
    rng = np.random.Generator(np.random.PCG64(11))
    cube = torch.from_numpy(rng.standard_normal((rows, cols, C_)).astype(np.float32)).to(DEV)
    X = torch.from_numpy(rng.standard_normal((rows * cols, bands)).astype(np.float32)).to(DEV)
    n = 777
    pix_h = rng.choice(rows * cols, n, replace=False)
    truth_h = rng.integers(0, K - 1, n)                     # the last class never occurs (CalAccuracy's max(label) + 1)
    truth_h[:K - 1] = np.arange(K - 1)
    pix, truth = torch.from_numpy(pix_h).to(DEV), torch.from_numpy(truth_h).to(DEV)
    eng = _trained_engine(shape)
    ev = Evaluator(NetShape(*shape), cube, X[pix].contiguous(), truth, pix)          # compact spectra, as scene_arrays()
    cm = ev.evaluate((eng, None))
    assert cm.shape == (2, K, K) and cm.dtype == torch.int64 and int(ev.ignored) == 0
    cm_h = cm.cpu().numpy().copy()
    again = ev.evaluate((eng, None)).cpu().numpy()
    assert cm_h.tobytes() == again.tobytes()
    for k in range(2):
        model = BaseNet2(num_features=bands, dropout=0.8, num_classes=K, in_channels=C_, window=H).to(DEV)
        model.load_state_dict(eng.state_dict(k))
        model.eval()
        pred = infer_cube(model, cube, X).cpu().numpy()[pix_h]
        want = np.zeros((K, K), dtype=np.int64)
        np.add.at(want, (truth_h, pred), 1)
        assert np.array_equal(cm_h[k], want), k                                   # exact counts
        OA, Kappa, prodA = CalAccuracy(pred, truth_h)
        oa, kappa, pa, aa = ev.metrics(cm[k])
        print(f"net {k}: OA {oa!r} / {OA!r}  Kappa {kappa!r} / {Kappa!r}  AA {aa!r} / {np.mean(prodA)!r}")
        np.testing.assert_allclose(oa, OA, rtol=RTOL, atol=0)
        np.testing.assert_allclose(kappa, Kappa, rtol=RTOL, atol=1e-15)
        np.testing.assert_allclose(pa, prodA, rtol=RTOL, atol=0)
        np.testing.assert_allclose(aa, np.mean(prodA), rtol=RTOL, atol=0)
        # one network of the engine, and the module, give that network's matrix
        assert np.array_equal(ev.evaluate((eng, k)).cpu().numpy()[0], want)
        assert np.array_equal(ev.evaluate(model).cpu().numpy()[0], want)
    # test_acc on the Evaluator: the reference's lines from the matrix (every class of 0 .. K - 2 occurs)
    capsys.readouterr()
    acc = test_acc((eng, 0), ev, 7, K - 1)
    out = capsys.readouterr().out
    np.testing.assert_allclose(acc, np.trace(cm_h[0]) / n, rtol=RTOL, atol=0)
    assert out.count("Accuracy of") == K - 1 and "Epoch[7]Validation-OA: %.2f %%" % (100.0 * acc) in out
    with pytest.raises(ValueError):
        Evaluator(NetShape(*shape), cube, X, truth, pix + rows * cols)                # a list outside the scene


EPOCH = re.compile(r"^Epoch \d+/\d+:  \d+/\d+ loss_contrast")
VAL = re.compile(r"^Epoch (\d+)/(\d+): validation(1?) OA = ([\d.]+) AA = ([\d.]+) Kappa = ([-\d.]+)$")
RESULT = re.compile(r"^ OA(1?)=([\d.]+),Kappa=([-\d.]+)$")


def _train(tmp_path, tag, *extra):
    hist = str(tmp_path / f"hist_{tag}.npy")
    r = subprocess.run([sys.executable, "train.py", "--synthetic", "B2", "--num_unlabel", "700", "--num_epochs", "3",
                        "--print_per_batches", "4", "--save_loss_hist", hist, *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines(), np.load(hist)


@pytest.mark.parametrize("mode", [(), ("--graph",), ("--windows", "cube"), ("--windows", "cube", "--graph")],
                         ids=["eager", "graph", "cube", "cube-graph"])
def test_train_py_eval_every(tmp_path, mode):
    npz = str(tmp_path / "eval.npz")
    base, hist0 = _train(tmp_path, "base", *mode)
    zero, hist00 = _train(tmp_path, "zero", "--eval_every", "0", *mode)
    out, hist1 = _train(tmp_path, "eval", "--eval_every", "1", "--save_eval", npz, *mode)
    # evaluation does not disturb training
    assert hist0.shape == (18, 5) and np.isfinite(hist0).all()
    assert np.array_equal(hist0, hist1) and np.array_equal(hist0, hist00)
    # without the option (or with 0): no evaluation line, the same Epoch lines, the same end-of-run block
    for lines in (base, zero):
        assert not any(VAL.match(ln) or ln.startswith("best validation") or ln.startswith("validation check") for ln in lines)
    timing = ("training:", "after the first epoch:", "inference time ==", "evaluation source ready")
    strip = lambda lines: [ln for ln in lines if not ln.startswith(timing)]
    assert strip(base) == strip(zero)
    assert [ln for ln in base if EPOCH.match(ln)] == [ln for ln in out if EPOCH.match(ln)]
    extra = lambda ln: bool(VAL.match(ln)) or ln.startswith(("best validation", "validation check"))
    assert strip(base) == [ln for ln in strip(out) if not extra(ln)]
    # three evaluations per network, in epoch order, after that epoch's lines
    vals = [VAL.match(ln) for ln in out if VAL.match(ln)]
    assert [(int(m.group(1)), m.group(3)) for m in vals] == [(1, ""), (1, "1"), (2, ""), (2, "1"), (3, ""), (3, "1")]
    z = np.load(npz)
    curve, cms = z["curve"], z["cm"]
    assert curve.shape == (3, 2, 3) and cms.shape == (3, 2, 9, 9) and list(z["epochs"]) == [1, 2, 3]
    assert (cms.sum((2, 3)) == 64 * 64).all()
    for i, m in enumerate(vals):
        e, k = divmod(i, 2)
        assert (m.group(4), m.group(5), m.group(6)) == tuple("%.2f" % (100 * v) for v in curve[e, k])
        np.testing.assert_allclose(curve[e, k, 0], np.trace(cms[e, k]) / cms[e, k].sum(), rtol=RTOL)
    # the last evaluation agrees with the end-of-run whole-image evaluation (both exact counts)
    res = [RESULT.match(ln) for ln in out if RESULT.match(ln)]
    assert len(res) == 2
    for k, m in enumerate(res):
        assert m.group(2) == "%.2f" % (100 * curve[2, k, 0]) and m.group(3) == "%.2f" % (100 * curve[2, k, 2])
    checks = [ln for ln in out if ln.startswith("validation check")]
    assert len(checks) == 2 and all("==" in ln and "!=" not in ln for ln in checks)
    best = [ln for ln in out if ln.startswith("best validation")]
    assert len(best) == 2
    for k, ln in enumerate(best):
        assert ln == "best validation%s: epoch %d OA = %.2f" % ("" if k == 0 else "1", 1 + int(np.argmax(curve[:, k, 0])),
                                                                100 * curve[:, k, 0].max())
