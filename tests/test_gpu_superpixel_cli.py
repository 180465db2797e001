"""GPU: the superpixel flags of the drivers (train.py --superpixel, predict.py --superpixel) on the synthetic B2 scene, one
epoch, from a checkpoint made here.  What the drivers write is held to the definitions in numpy
(cmlpl_amd.superpixel.segment_host / region_vote_host) exactly."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cmlpl_amd.superpixel import asa, region_vote_host, segment_host
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["--synthetic", "B2", "--synthetic_scene", "--num_epochs", "1", "--num_unlabel", "128", "--labeled_batch_size", "32",
       "--unlabeled_batch_size", "32", "--print_per_batches", "2"]
STATS = re.compile(r"^superpixel: segments=(\d+) empty=(\d+) mean_size=(\S+) max_size=(\d+) ASA=(\S+)$")
ROWS = COLS = 64                    # the synthetic scene of train.py / predict.py --synthetic


def _py(script, *args, ok=True):
    r = subprocess.run([sys.executable, script, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return r.stdout.splitlines()
    return r


def _timeless(lines):
    return [ln for ln in lines if " time == " not in ln and " steps in " not in ln and " ready in " not in ln]


def _oa_tags(lines):
    return [ln.split("=")[0] for ln in lines if ln.startswith(" OA")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sp"))
    f = lambda name: os.path.join(d, name)
    # (a checkpoint records the run's command line, paths included: both runs write the SAME paths, one after the other)
    files = ["--save_loss_hist", f("hist.npy"), "--save_ckpt", f("run.pt")]
    plain = _py("train.py", *RUN, *files)
    for name in ("hist.npy", "run.pt"):
        os.replace(f(name), f("plain_" + name))
    with_sp = _py("train.py", *RUN, "--superpixel", "4", "--save_segments", f("train_seg.npy"), *files)
    return dict(with_sp=with_sp, plain=plain, f=f)


@pytest.fixture(scope="module")
def scene():
    """the scene's cube and truth, and the definition's map of it at S = 4 with the defaults"""
    import train
    from hsi_loader import SyntheticScene
    whole = SyntheticScene(train.SYNTH["B2"], ROWS, COLS, seed=3)
    cube = whole.cube_source(torch.device(DEV)).cube.cpu().numpy()
    assert cube.shape[:2] == (ROWS, COLS)
    return dict(cube=cube, Y=whole.Y.numpy(), K=train.SYNTH["B2"][4], ref=segment_host(cube, 4, 1.0, 10, 3))


def _check_stats(lines, ref, Y, K):
    stats = [STATS.match(ln) for ln in lines if ln.startswith("superpixel:")]
    assert len(stats) == 1 and stats[0] is not None, [ln for ln in lines if ln.startswith("superpixel")]
    N, counts = ref["ny"] * ref["nx"], ref["counts"]
    want = (str(N), str(int((counts == 0).sum())), "%.1f" % (counts.sum() / N), str(counts.max()),
            "%.4f" % asa(ref["seg"], N, np.arange(ROWS * COLS), Y, K))
    assert stats[0].groups() == want


def test_train_adds_exactly_its_lines_and_leaves_the_run_alone(runs, scene):
    out, plain, f = runs["with_sp"], runs["plain"], runs["f"]
    assert _oa_tags(out) == [" OA", " OA1", " OA_ens_sp"] and _oa_tags(plain) == [" OA", " OA1"]
    assert sum(ln.startswith("producerA_ens_sp:") for ln in out) == 1 and sum(ln.startswith("AA_ens_sp=") for ln in out) == 1
    assert sum("superpixel time ==" in ln and "step 4" in ln for ln in out) == 1
    assert np.load(f("hist.npy")).tobytes() == np.load(f("plain_hist.npy")).tobytes()         # loss_hist bit-equal
    assert open(f("run.pt"), "rb").read() == open(f("plain_run.pt"), "rb").read()              # the checkpoint, every byte
    assert not any("superpixel" in ln or "_sp" in ln for ln in plain)
    i = next(k for k, ln in enumerate(out) if ln.startswith("ensemble inference time"))
    assert _timeless(out[:i]) == _timeless(plain) and len(out) - i <= 12                       # every other line as it was
    _check_stats(out, scene["ref"], scene["Y"], scene["K"])
    assert np.array_equal(np.load(f("train_seg.npy")), scene["ref"]["seg"])


def test_predict_ensemble_with_superpixels(runs, scene):
    f, ref, K = runs["f"], scene["ref"], scene["K"]
    n, N = ROWS * COLS, scene["ref"]["ny"] * scene["ref"]["nx"]
    got = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", "--net", "ensemble", "--superpixel", "4", "--save_segments",
              f("seg.npy"), "--out", f("lab.npy"), "--proba", f("q.npy"), "--confidence", f("c.npy"), "--entropy", f("e.npy"))
    raw = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", "--net", "ensemble", "--out", f("lab0.npy"), "--proba", f("p.npy"))
    assert _oa_tags(got) == [" OA_ens", " OA_ens_sp"] and _oa_tags(raw) == [" OA_ens"]
    results = lambda lines: [ln for ln in lines if ln.startswith(("Result:", " OA", "producerA", "AA")) or ln.startswith("[")]
    assert results(got)[:len(results(raw))] == results(raw)                 # the raw block is printed as it is without the flag
    assert not any("superpixel" in ln for ln in raw)
    _check_stats(got, ref, scene["Y"], K)
    seg, lab, q, c, e, p = (np.load(f(x)) for x in ("seg.npy", "lab.npy", "q.npy", "c.npy", "e.npy", "p.npy"))
    assert seg.dtype == np.int32 and np.array_equal(seg, ref["seg"])
    want = region_vote_host(ref["seg"], N, K, probs=p)
    assert lab.dtype == np.int64 and np.array_equal(lab, want["labels"])
    assert q.dtype == np.float32 and q.shape == (n, K) and np.array_equal(q.view(np.int32), want["probs"].view(np.int32))
    assert np.array_equal(c.view(np.int32), want["conf"].view(np.int32)) and e.shape == (n,) and (e >= 0).all()
    # the block is the vote's score, and the one train.py printed for the same networks
    oa = 100 * (want["labels"] == scene["Y"]).mean()
    assert [ln for ln in got if ln.startswith(" OA_ens_sp=")][0].startswith(" OA_ens_sp=%.2f," % oa)
    assert [ln for ln in got if ln.startswith(" OA_ens_sp")] == [ln for ln in runs["with_sp"] if ln.startswith(" OA_ens_sp")]


def test_predict_stages_compose_in_order(runs):
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", "--net", "ensemble", "--smooth", "2", "--superpixel", "4",
              "--temperature", "2", "--reliability", "--out", f("labT.npy"), "--proba", f("qT.npy"))
    tags = ["_ens", "_ens_smooth", "_ens_smooth_sp", "_ens_smooth_sp_T"]
    assert _oa_tags(got) == [" OA" + t for t in tags]
    marks = [ln.split("=")[0].strip() if ln.startswith(" OA") else ln.split(":")[0] for ln in got
             if ln.startswith((" OA", "Reliability"))]
    assert marks == [m for t in tags for m in ("OA" + t, "Reliability" + t)]       # every block, its line behind it
    at = lambda s: next(k for k, ln in enumerate(got) if s in ln)
    assert at("smoothing time ==") < at("superpixel:") < at("superpixel time ==") < at("tempering time ==")
    lab, q = np.load(f("labT.npy")), np.load(f("qT.npy"))
    assert np.array_equal(lab, q.argmax(1)) and np.abs(q.sum(1) - 1).max() < 1e-5              # the LAST stage's outputs


def test_predict_one_network_with_tta_and_a_hard_vote(runs, scene):
    f, K = runs["f"], scene["K"]
    got = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", "--net", "1", "--tta", "2", "--superpixel", "8", "--sp_vote",
              "hard", "--sp_guide", "0", "--sp_iters", "2", "--save_segments", f("seg8.npy"), "--out", f("lab8.npy"), "--proba", f("q8.npy"))
    assert _oa_tags(got) == [" OA_tta", " OA_tta_sp"]
    seg, lab, q = np.load(f("seg8.npy")), np.load(f("lab8.npy")), np.load(f("q8.npy"))
    grid = segment_host(scene["cube"], 8, 1.0, 2, 0)
    assert np.array_equal(seg, grid["seg"]) and grid["counts"].sum() == ROWS * COLS            # no guide: the image distance alone
    votes = q.astype(np.float64) * grid["counts"][seg][:, None]                                # a hard vote's q: counts over the segment
    assert np.array_equal(lab, q.argmax(1)) and np.abs(votes - np.round(votes)).max() < 1e-3
    assert np.abs(votes.sum(1) - grid["counts"][seg]).max() < 1e-3
    first = np.unique(seg, return_index=True)[1]
    assert np.array_equal(q, q[first][seg])                                                    # one row per segment


def test_what_the_command_lines_refuse(runs):
    f = runs["f"]
    # (every other refusal is held in-process by tests/test_superpixel_host.py: each of these starts an interpreter)
    for more, word in ((["--net", "both", "--superpixel", "4"], "--net both"), (["--superpixel", "4", "--knn", "3"], "--knn")):
        r = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", *more, ok=False)
        assert r.returncode != 0 and word in r.stderr, (more, r.stderr[-500:])
