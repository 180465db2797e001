"""GPU: the propagation flags of the drivers (train.py --propagate, predict.py --propagate) on the synthetic B2 scene, one
epoch, from a checkpoint made here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cmlpl_amd.labelprop import LabelProp, propagate_embedding, score_labels
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["--synthetic", "B2", "--synthetic_scene", "--num_epochs", "1", "--num_unlabel", "128", "--labeled_batch_size", "32",
       "--unlabeled_batch_size", "32", "--print_per_batches", "2", "--no_eval"]
LINE = re.compile(r"^Epoch 1/1: validation_lp(1?) OA = (\S+) AA = (\S+) Kappa = (\S+)$")
PROP = re.compile(r"^propagate(1?): nodes=(\d+) edges=(\d+) max_in_degree=(\d+) unreached=(\d+) residual=(\S+)$")


def _py(script, *args, ok=True):
    r = subprocess.run([sys.executable, script, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return r.stdout.splitlines()
    return r


def _timeless(lines):
    return [ln for ln in lines if " time == " not in ln and " steps in " not in ln and " ready in " not in ln]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lp"))
    f = lambda name: os.path.join(d, name)
    # (a checkpoint records the run's command line, paths included: both runs write the SAME paths, one after the other)
    files = ["--save_loss_hist", f("hist.npy"), "--save_ckpt", f("run.pt")]
    plain = _py("train.py", *RUN, *files)
    for name in ("hist.npy", "run.pt"):
        os.replace(f(name), f("plain_" + name))
    with_lp = _py("train.py", *RUN, "--propagate", *files)
    return dict(with_lp=with_lp, plain=plain, f=f)


def _nodes(ckpt):
    import train
    from cmlpl_amd import checkpoint
    from hsi_loader import SyntheticHSIDataSet, SyntheticScene
    ck = checkpoint.load(ckpt)
    shape = train.SYNTH["B2"]
    scene = SyntheticScene(shape, 64, 64, seed=3)
    lab = SyntheticHSIDataSet(shape, 128, 'label', seed=1, scene=scene)
    models = train.build_nets(shape, [(0, ck["Base"]), (1, ck["Base1"])], torch.device(DEV), ck["identity"]["hp"]["dropout"])
    for m in models:
        m.eval()
    spectra, seeds = train.propagate_nodes(lab.X, lab.Y, scene.X, torch.device(DEV))
    return shape, models, spectra, seeds, scene.Y.numpy()


def test_train_only_adds_the_two_lines(runs):
    out, plain, f = runs["with_lp"], runs["plain"], runs["f"]
    lines = [ln for ln in out if "validation_lp" in ln]
    print("\n".join(lines))
    assert [LINE.match(ln).group(1) for ln in lines] == ["", "1"]
    assert np.load(f("hist.npy")).tobytes() == np.load(f("plain_hist.npy")).tobytes()         # loss_hist bit-equal
    assert open(f("run.pt"), "rb").read() == open(f("plain_run.pt"), "rb").read()              # the checkpoint, every byte
    assert _timeless([ln for ln in out if "validation_lp" not in ln]) == _timeless(plain)      # every other line as it was
    assert not any("validation_lp" in ln or "propagate" in ln for ln in plain)
    # the lines are label_propagation of the run's final networks on the same nodes
    shape, models, spectra, seeds, truth = _nodes(f("run.pt"))
    with torch.no_grad():
        pairs = propagate_embedding(tuple(models), spectra, seeds, shape[4], LabelProp(), probs=False)
    for net, (_, res) in enumerate(pairs):
        OA, Kappa, _, AA, _ = score_labels(res.labels[len(seeds) - len(truth):].cpu().numpy(), truth, shape[4])
        assert lines[net] == 'Epoch 1/1: validation_lp%s OA = %.2f AA = %.2f Kappa = %.2f' % ("1" if net else "", OA * 100, AA * 100, Kappa * 100)


def test_predict_propagate_both_networks_with_knn(runs):
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", "--net", "both", "--knn", "10", "--propagate", "--lp_k", "8",
              "--lp_iters", "30")
    print("\n".join(got))
    heads = [ln for ln in got if ln.startswith(" OA")]
    assert [h.split("=")[0] for h in heads] == [" OA_knn", " OA_knn1", " OA_lp", " OA_lp1"]             # _knn first, then _lp
    assert got.count("Result:") == 4
    shape, models, spectra, seeds, truth = _nodes(f("run.pt"))
    first = len(seeds) - len(truth)
    props = [PROP.match(ln) for ln in got if ln.startswith("propagate")]
    assert [m.group(1) for m in props] == ["", "1"]
    with torch.no_grad():
        pairs = propagate_embedding(tuple(models), spectra, seeds, shape[4], LabelProp(k=8, iters=30), residual=True)
    for net, (graph, res) in enumerate(pairs):
        labels = res.labels[first:].cpu().numpy()
        OA, Kappa, producerA, AA, cm = score_labels(labels, truth, shape[4])
        tag = "_lp" + ("1" if net else "")
        assert heads[2 + net] == " OA%s=%.2f,Kappa=%.2f" % (tag, OA * 100, Kappa * 100)
        assert "AA%s=%.2f" % (tag, AA * 100) in got
        assert cm.sum() == len(truth) == 4096 and cm[:, -1].sum() == (labels < 0).sum()
        m = props[net]
        assert [int(v) for v in m.group(2, 3, 4, 5)] == [len(seeds), graph.edges(), graph.max_in_degree(), int((labels < 0).sum())]
        assert m.group(6) == "%.3e" % float(res.residual.cpu()[0])


def test_predict_propagate_one_network_with_reliability(runs):
    from cmlpl_amd.calibrate import reliability
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", "--net", "1", "--propagate", "--reliability")
    shape, models, spectra, seeds, truth = _nodes(f("run.pt"))
    with torch.no_grad():
        _, res = propagate_embedding(models[1], spectra, seeds, shape[4], LabelProp())[0]
    j = [n for n, ln in enumerate(got) if ln.startswith("AA_lp1=")][0]
    probs = res.probs[len(seeds) - len(truth):].clone()
    assert got[j + 1] == reliability(probs, torch.from_numpy(truth).to(DEV), None, 15).line("_lp1")
    assert got.count("Result:") == 1 and len([ln for ln in got if ln.startswith("propagate1: ")]) == 1


def test_the_drivers_refuse_what_propagate_cannot_mean(runs):
    """(every refusal is in tests/test_labelprop_host.py, on the argument checks themselves; here: that the programs exit)"""
    f = runs["f"]
    r = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", "--propagate", "--out", f("x.npy"), ok=False)
    assert r.returncode != 0 and "not the scene" in r.stderr and "Result:" not in r.stdout and not os.path.exists(f("x.npy"))
    r = _py("train.py", *RUN, "--lp_gamma", "2", ok=False)
    assert r.returncode != 0 and "belongs to --propagate" in r.stderr and "Epoch" not in r.stdout
