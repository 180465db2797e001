"""GPU: the calibration flags of the drivers (predict.py --reliability / --temperature, train.py --reliability) on the small
synthetic scene, from a checkpoint made here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cmlpl_amd import calibrate as cal
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["--synthetic", "W8", "--num_epochs", "1", "--synthetic_scene", "--num_unlabel", "128", "--labeled_batch_size", "32",
       "--unlabeled_batch_size", "32", "--print_per_batches", "2"]
RESULT = ("Result:", " OA", "producerA", "AA")
N, K = 64 * 64, 5                                           # the synthetic scene: every pixel is a labelled test pixel
LINE = re.compile(r"^Reliability(\S*): ECE=(\S+) MCE=(\S+) NLL=(\S+) Brier=(\S+) conf=(\S+) acc=(\S+)( \(held-out n=(\d+)\))?$")


def _py(script, *args):
    r = subprocess.run([sys.executable, script, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _timeless(lines):
    return [ln for ln in lines if " time == " not in ln and " steps in " not in ln and " ready in " not in ln]


def _rel_lines(lines):
    return [ln for ln in lines if ln.startswith("Reliability")]


def _truth():
    import train
    from hsi_loader import SyntheticScene
    return SyntheticScene(train.SYNTH["W8"], 64, 64, seed=3).Y.numpy().astype(np.int64)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("calib"))
    f = lambda name: os.path.join(d, name)
    out = _py("train.py", *RUN, "--ensemble", "--reliability", "--save_loss_hist", f("R.npy"), "--save_ckpt", f("R.pt"))
    plain = _py("train.py", *RUN, "--ensemble", "--save_loss_hist", f("plain.npy"), "--save_ckpt", f("P.pt"))
    pred = _py("predict.py", "--ckpt", f("R.pt"), "--synthetic", "W8", "--net", "ensemble", "--out", f("lab0.npy"), "--proba", f("p0.npy"))
    return dict(out=out, plain=plain, pred=pred, f=f)


def test_train_with_reliability_adds_one_line_and_leaves_the_run_alone(runs):
    out, plain, f = runs["out"], runs["plain"], runs["f"]
    assert np.load(f("R.npy")).tobytes() == np.load(f("plain.npy")).tobytes()             # loss_hist bit-equal
    rel = _rel_lines(out)
    print("\n".join(rel))
    assert len(rel) == 1 and LINE.match(rel[0]).group(1) == "_ens" and LINE.match(rel[0]).group(8) is None
    assert _timeless([ln for ln in out if not ln.startswith("Reliability")]) == _timeless(plain)
    assert not any("Reliability" in ln or "temperature" in ln for ln in plain)
    i = out.index(rel[0])
    assert out[i - 1].startswith("AA_ens=")                                             # behind its Result: block
    r = subprocess.run([sys.executable, "train.py", *RUN, "--reliability"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--ensemble, --tta or --smooth" in r.stderr and "Epoch" not in r.stdout


def test_predict_reliability_line_is_the_library_call_on_the_written_probabilities(runs):
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("R.pt"), "--synthetic", "W8", "--net", "ensemble", "--reliability", "--proba", f("p.npy"),
              "--save_reliability", f("rel.npz"), "--out", f("lab.npy"))
    plain = runs["pred"]
    rel = _rel_lines(got)
    assert len(rel) == 1 and rel[0].startswith("Reliability_ens: ") and got[got.index(rel[0]) - 1].startswith("AA_ens=")
    assert rel == _rel_lines(runs["out"])                                               # train.py's report scored the same networks
    p = np.load(f("p.npy"))
    assert p.shape == (N, K) and p.dtype == np.float32
    want = cal.reliability(torch.from_numpy(p).to(DEV), torch.from_numpy(_truth()).to(DEV), torch.arange(N, device=DEV), 15)
    assert rel[0] == want.line("_ens") and want.items == N and want.known == N
    saved = np.load(f("rel.npz"))
    assert list(saved) == ["Reliability_ens"] and np.array_equal(saved["Reliability_ens"], want.counts)
    exact = [0, 1, 2, 3, 4, 5, 7] + list(range(cal.REL_HEAD, cal.rel_size(15)))
    assert np.array_equal(cal.reliability_host(p, _truth(), None, 15).counts[exact], want.counts[exact])
    assert np.array_equal(p, np.load(f("p0.npy")))
    # without the flags: the parent's output, line for line
    assert _timeless(plain) == _timeless([ln for ln in got if not ln.startswith("Reliability")])
    assert not any("Reliability" in ln or "temperature" in ln for ln in plain)
    assert np.array_equal(np.load(f("lab.npy")), np.load(f("lab0.npy")))
    # 1024 bins: the same head, the risk-coverage curve's resolution
    fine = _py("predict.py", "--ckpt", f("R.pt"), "--synthetic", "W8", "--net", "ensemble", "--reliability", "--rel_bins", "1024",
               "--save_reliability", f("rel1024.npz"))
    blk = cal.Reliability(np.load(f("rel1024.npz"))["Reliability_ens"])
    assert blk.bins == 1024 and np.array_equal(blk.counts[:cal.REL_HEAD], want.counts[:cal.REL_HEAD]) and len(_rel_lines(fine)) == 1
    cov, acc = blk.risk_coverage()
    assert cov[-1] == 1.0 and acc[-1] == want.accuracy


def test_predict_temperature_fit_is_seeded_held_out_and_keeps_the_labels(runs):
    f = runs["f"]
    args = ["predict.py", "--ckpt", f("R.pt"), "--synthetic", "W8", "--net", "ensemble", "--reliability", "--temperature", "fit",
            "--calib_seed", "5", "--calib_frac", "0.3"]
    a = _py(*args, "--out", f("labT.npy"), "--proba", f("q.npy"), "--confidence", f("c.npy"))
    b = _py(*args)
    rel = _rel_lines(a)
    print("\n".join(ln for ln in a if ln.startswith(("Reliability", "temperature"))))
    assert rel == _rel_lines(b) and [LINE.match(ln).group(1) for ln in rel] == ["_ens", "_ens_T"]
    assert all(int(LINE.match(ln).group(9)) == N - int(round(0.3 * N)) for ln in rel)
    t = [ln for ln in a if ln.startswith("temperature = ")]
    assert len(t) == 1 and t == [ln for ln in b if ln.startswith("temperature = ")]
    m = re.match(r"^temperature = (\d+\.\d{4}) \(NLL (\d+\.\d{4}) -> (\d+\.\d{4}) on the calibration share\)$", t[0])
    assert m and 1 / 16 <= float(m.group(1)) <= 16 and float(m.group(3)) <= float(m.group(2))
    assert [ln.split("=")[0] for ln in a if ln.startswith(" OA")] == [" OA_ens", " OA_ens_T"]
    oa = [ln.split("=", 1)[1] for ln in a if ln.startswith(" OA")]
    assert oa[0] == oa[1]                                                                # the same labels, the same accuracy
    q, c, lab = np.load(f("q.npy")), np.load(f("c.npy")), np.load(f("labT.npy"))
    assert np.array_equal(lab, np.load(f("lab0.npy")))                                   # the _T labels are the untempered ones
    assert np.array_equal(c, q[np.arange(N), lab]) and np.array_equal(c, q.max(axis=1))
    # the held-out line is the library call on the held-out pixels of the written probabilities
    import train
    fit, held = train.calibration_split(N, 0.3, 5)
    want = cal.reliability(torch.from_numpy(q).to(DEV), torch.from_numpy(_truth()[held]).to(DEV),
                           torch.from_numpy(held.astype(np.int64)).to(DEV), 15)
    assert rel[1] == want.line("_ens_T", " (held-out n=%d)" % len(held))
    # the fitted T is the library's on the calibration share of the untempered probabilities
    T, before, after = cal.fit_temperature(torch.from_numpy(np.load(f("p0.npy"))).to(DEV), torch.from_numpy(_truth()[fit]).to(DEV),
                                           torch.from_numpy(fit.astype(np.int64)).to(DEV))
    assert t[0] == "temperature = %.4f (NLL %.4f -> %.4f on the calibration share)" % (T, before, after)


def test_predict_smooth_then_temperature_prints_three_blocks_in_order(runs):
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("R.pt"), "--synthetic", "W8", "--net", "ensemble", "--smooth", "2", "--temperature", "2",
              "--reliability", "--entropy", f("e.npy"))
    assert [ln.split("=")[0] for ln in got if ln.startswith(" OA")] == [" OA_ens", " OA_ens_smooth", " OA_ens_smooth_T"]
    rel = _rel_lines(got)
    assert [LINE.match(ln).group(1) for ln in rel] == ["_ens", "_ens_smooth", "_ens_smooth_T"]
    assert rel[0] == _rel_lines(runs["out"])[0] and sum("tempering time ==" in ln and "T 2" in ln for ln in got) == 1
    order = [k for k, ln in enumerate(got) if ln.startswith((" OA", "Reliability"))]
    assert [got[k][:3] for k in order] == [" OA", "Rel"] * 3
    # T = 2 flattens: the confidence falls, the entropy rises, the accuracy stays
    conf = [float(LINE.match(ln).group(6)) for ln in rel]
    assert conf[2] < conf[1] and LINE.match(rel[2]).group(7) == LINE.match(rel[1]).group(7)
    e = np.load(f("e.npy"))
    assert e.shape == (N,) and (e >= 0).all()


def test_predict_one_network_scores_and_tempers_its_own_softmax(runs):
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("R.pt"), "--synthetic", "W8", "--net", "1", "--reliability", "--temperature", "1.5",
              "--proba", f("q1.npy"))
    assert [ln.split("=")[0] for ln in got if ln.startswith(" OA")] == [" OA1", " OA1_T"]
    assert [LINE.match(ln).group(1) for ln in _rel_lines(got)] == ["1", "1_T"]
    assert [ln for ln in got if ln.startswith(" OA1=")] == [ln for ln in runs["out"] if ln.startswith(" OA1=")]
    q = np.load(f("q1.npy"))
    want = cal.reliability(torch.from_numpy(q).to(DEV), torch.from_numpy(_truth()).to(DEV), None, 15)
    assert _rel_lines(got)[1] == want.line("1_T")
