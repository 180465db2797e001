"""GPU: the kNN flags of the drivers (train.py --knn, predict.py --knn / --knn_gallery / --embed) on the synthetic B2 scene,
two epochs, from checkpoints made here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["--synthetic", "B2", "--synthetic_scene", "--num_epochs", "2", "--num_unlabel", "128", "--labeled_batch_size", "32",
       "--unlabeled_batch_size", "32", "--print_per_batches", "2", "--no_eval"]
LINE = re.compile(r"^Epoch (\d)/2: validation_knn(1?) OA = (\S+) AA = (\S+) Kappa = (\S+)$")


def _py(script, *args):
    r = subprocess.run([sys.executable, script, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _timeless(lines):
    return [ln for ln in lines if " time == " not in ln and " steps in " not in ln and " ready in " not in ln]


def _knn_lines(lines):
    return [ln for ln in lines if "validation_knn" in ln]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("knn"))
    f = lambda name: os.path.join(d, name)
    with_knn = _py("train.py", *RUN, "--eval_every", "1", "--knn", "5", "--save_loss_hist", f("A.npy"), "--save_eval", f("A.npz"),
                   "--save_ckpt", f("A{epoch}.pt"), "--ckpt_every", "1")
    plain = _py("train.py", *RUN, "--eval_every", "1", "--save_loss_hist", f("B.npy"), "--save_eval", f("B.npz"),
                "--save_ckpt", f("B.pt"))
    return dict(with_knn=with_knn, plain=plain, f=f)


def test_train_prints_the_lines_and_leaves_the_run_alone(runs):
    out, plain, f = runs["with_knn"], runs["plain"], runs["f"]
    lines = _knn_lines(out)
    print("\n".join(lines))
    assert [LINE.match(ln).group(1, 2) for ln in lines] == [("1", ""), ("1", "1"), ("2", ""), ("2", "1")]
    assert np.load(f("A.npy")).tobytes() == np.load(f("B.npy")).tobytes()                   # loss_hist bit-equal
    assert _timeless([ln for ln in out if "validation_knn" not in ln]) == _timeless(plain)    # every other line as it was
    assert not _knn_lines(plain)
    a, b = np.load(f("A.npz")), np.load(f("B.npz"))
    assert list(a) == list(b) + ["curve_knn", "cm_knn", "epochs_knn"]
    assert all(np.array_equal(a[k], b[k]) for k in b)
    assert a["curve_knn"].shape == (2, 2, 3) and a["cm_knn"].shape == (2, 2, 9, 9) and a["epochs_knn"].tolist() == [1, 2]
    assert a["cm_knn"].sum(axis=(2, 3)).tolist() == [[4096, 4096]] * 2                       # every test pixel has a neighbour
    for e in range(2):
        for net in range(2):
            assert lines[2 * e + net] == 'Epoch %d/2: validation_knn%s OA = %.2f AA = %.2f Kappa = %.2f' % (
                e + 1, "1" if net else "", *(100 * a["curve_knn"][e, net]))
    # the curve goes into checkpoints only with the flag
    from cmlpl_amd import checkpoint
    ex_a, ex_b = checkpoint.load(f("A2.pt"))["extra"], checkpoint.load(f("B.pt"))["extra"]
    assert [int(e) for e in ex_a["eval_epochs_knn"]] == [1, 2] and np.array_equal(ex_a["eval_curve_knn"].numpy(), a["curve_knn"])
    assert not any("knn" in k for k in ex_b) and not any("knn" in k for k in ex_b["args"])
    assert ex_a["args"]["knn"] == 5


def test_resume_restores_the_curve(runs):
    f = runs["f"]
    out = _py("train.py", *RUN, "--eval_every", "1", "--knn", "5", "--resume", f("A1.pt"), "--save_loss_hist", f("R.npy"),
              "--save_eval", f("R.npz"))
    a, r = np.load(f("A.npz")), np.load(f("R.npz"))
    assert r["epochs_knn"].tolist() == [1, 2]
    assert np.array_equal(r["curve_knn"], a["curve_knn"]) and np.array_equal(r["cm_knn"], a["cm_knn"])
    assert np.load(f("R.npy")).tobytes() == np.load(f("A.npy")).tobytes()
    assert _knn_lines(out) == _knn_lines(runs["with_knn"])[2:]                               # epoch 2's lines, once


def test_train_without_eval_every_prints_the_lines_once_after_the_last_epoch(runs):
    out = _py("train.py", *RUN, "--knn", "5")
    assert _knn_lines(out) == _knn_lines(runs["with_knn"])[2:]
    r = subprocess.run([sys.executable, "train.py", *RUN, "--knn", "33"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--knn K" in r.stderr and "Epoch" not in r.stdout


def _inputs(ckpt):
    import train
    from cmlpl_amd import checkpoint
    from hsi_loader import SyntheticScene
    ck = checkpoint.load(ckpt)
    shape = train.SYNTH["B2"]
    scene = SyntheticScene(shape, 64, 64, seed=3)
    models = train.build_nets(shape, [(0, ck["Base"]), (1, ck["Base1"])], torch.device(DEV), ck["identity"]["hp"]["dropout"])
    for m in models:
        m.eval()
    return shape, ck, models, scene.X.to(DEV).contiguous(), scene.Y.to(DEV).contiguous()


def test_predict_knn_loo_reliability_and_embed(runs):
    from cmlpl_amd import NetShape
    from cmlpl_amd.calibrate import reliability
    from cmlpl_amd.evaluate import metrics
    from cmlpl_amd.knn import KnnEvaluator, embed
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("A2.pt"), "--synthetic", "B2", "--knn", "5", "--knn_gallery", "loo", "--reliability",
              "--embed", f("feat.npy"))
    print("\n".join(got))
    shape, ck, models, X, Y = _inputs(f("A2.pt"))
    ev = KnnEvaluator(NetShape(*shape), X, Y, k=5, T=ck["identity"]["hp"]["temperature"], loo=True)
    OA, Kappa, producerA, AA = metrics(ev.evaluate(models[0])[0])
    i = got.index("Result:")
    assert got[i + 1] == " OA_knn=%.2f,Kappa=%.2f" % (OA * 100, Kappa * 100)
    assert got[i + 2].startswith("producerA_knn:")
    j = [n for n, ln in enumerate(got) if ln.startswith("AA_knn=")][0]
    assert got[j] == "AA_knn=%.2f" % (AA * 100)
    assert got[j + 1] == reliability(ev.last.probs[0], Y, None, 15).line("_knn")
    assert got.count("Result:") == 1 and len([ln for ln in got if ln.startswith("Reliability")]) == 1
    feat = np.load(f("feat.npy"))
    assert feat.dtype == np.float32 and feat.shape == (4096, 1024)
    assert np.array_equal(feat, embed(models[0], X)[0].cpu().numpy())
    assert bool((ev.last.labels[0] >= 0).all())


def test_predict_knn_over_the_training_pixels_both_networks(runs):
    import train
    from cmlpl_amd import NetShape
    from cmlpl_amd.evaluate import metrics
    from cmlpl_amd.knn import KnnEvaluator
    from hsi_loader import SyntheticHSIDataSet, SyntheticScene
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("A2.pt"), "--synthetic", "B2", "--net", "both", "--knn", "5", "--knn_T", "0.1")
    shape, ck, models, X, Y = _inputs(f("A2.pt"))
    lab = SyntheticHSIDataSet(shape, 128, 'label', seed=1, scene=SyntheticScene(shape, 64, 64, seed=3))
    ev = KnnEvaluator(NetShape(*shape), lab.X.to(DEV).contiguous(), lab.Y.to(DEV).contiguous(), X, Y, k=5, T=0.1)
    cms = ev.evaluate(tuple(models))
    heads = [ln for ln in got if ln.startswith(" OA")]
    assert heads == [" OA_knn%s=%.2f,Kappa=%.2f" % (tag, metrics(cm)[0] * 100, metrics(cm)[1] * 100) for tag, cm in zip(("", "1"), cms)]
    # train.py's last line of the same networks scored the same lists at the run's own temperature
    ev3 = KnnEvaluator(NetShape(*shape), lab.X.to(DEV).contiguous(), lab.Y.to(DEV).contiguous(), X, Y, k=5, T=0.3)
    OA = metrics(ev3.evaluate(models[0])[0])[0]
    assert LINE.match(_knn_lines(runs["with_knn"])[2]).group(3) == "%.2f" % (OA * 100)


def test_predict_refuses_what_knn_cannot_mean(runs):
    f = runs["f"]
    for extra, word in ((["--net", "ensemble", "--knn", "5"], "ONE network"), (["--knn_T", "0.1"], "belong to --knn"),
                        (["--knn", "5", "--out", f("x.npy")], "not the scene"), (["--net", "both", "--embed", f("x.npy")], "single network")):
        r = subprocess.run([sys.executable, "predict.py", "--ckpt", f("A2.pt"), "--synthetic", "B2", *extra], cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and word in r.stderr and "Result:" not in r.stdout, (extra, r.stderr[-500:])
