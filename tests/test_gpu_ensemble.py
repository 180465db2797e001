"""GPU: the ensemble kernel against its definition in fp64 (tests/test_ensemble_host.py), its exact rules bit for bit, the
host functions against each other and against the eval forwards they are made of, and the two command lines.

Tolerances.  Probabilities, confidence and entropy: the yardstick is the error of the SAME arithmetic in fp32 by torch on
the CPU against fp64 on the same inputs (0.8 .. 2.9e-7 for p, 1 .. 5e-7 for the entropy on these inputs); the device is
allowed 8 x that per case, because its expf / logf are not libm's and its sums run in butterfly order.  Labels: equal
wherever the fp64 top-2 margin of p is >= 1e-5, which may leave out at most 1 % of a case (the reference leaves out at
most 0.2 %).  Disagreement: exact where every member's own margin is >= 1e-5 as well."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV
from tests.test_ensemble_host import (case_logits, ensemble_fp32_torch, ensemble_fp64, first_max, normalised_weights,
                                      top2_margin)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-5


def _run(z, weights=None, stride_pad=0):
    """the kernel on logits [M, n, K] (numpy): every output, as numpy"""
    from cmlpl_amd.ensemble import ensemble_logits
    M, n, K = z.shape
    if stride_pad:
        buf = torch.full((M, n * K + stride_pad), float("nan"), dtype=torch.float32, device=DEV)
        buf[:, :n * K] = torch.from_numpy(z.reshape(M, n * K)).to(DEV)
        zt = buf[:, :n * K].view(M, n, K)
        assert zt.stride(0) == n * K + stride_pad
    else:
        zt = torch.from_numpy(z).to(DEV)
    r = ensemble_logits(zt, weights=weights, probs=True, conf=True, entropy=True, disagree=True)
    torch.cuda.synchronize()
    assert r.labels.dtype == torch.int64 and r.disagree.dtype == torch.int32 and r.probs.shape == (n, K)
    return {k: getattr(r, k).cpu().numpy() for k in ("labels", "probs", "conf", "entropy", "disagree")}


def _check_against_fp64(z, weights=None, stride_pad=0, tag=""):
    ref = ensemble_fp64(z, weights)
    p32, e32 = ensemble_fp32_torch(z, weights)
    tol_p = 8 * np.abs(p32 - ref["p"]).max()
    tol_e = 8 * np.abs(e32 - ref["entropy"]).max()
    got = _run(z, weights, stride_pad)
    err_p = np.abs(got["probs"] - ref["p"]).max()
    err_c = np.abs(got["conf"] - ref["conf"]).max()
    err_e = np.abs(got["entropy"] - ref["entropy"]).max()
    sure = top2_margin(ref["p"]) >= MARGIN
    sure_m = sure & (top2_margin(ref["pm"]) >= MARGIN).all(0)
    print("%s M %d K %d: p err %.2e (allowed %.2e) conf err %.2e entropy err %.2e (allowed %.2e) under the margin %.4f"
          % (tag, z.shape[0], z.shape[2], err_p, tol_p, err_c, err_e, tol_e, 1 - sure.mean()))
    assert err_p <= tol_p and err_c <= tol_p and err_e <= tol_e
    assert sure.mean() >= 0.99
    assert np.array_equal(got["labels"][sure], ref["label"][sure])
    assert np.array_equal(got["disagree"][sure_m], ref["disagree"][sure_m])
    assert ((got["labels"] >= 0) & (got["labels"] < z.shape[2])).all()
    assert ((got["disagree"] >= 0) & (got["disagree"] <= z.shape[0])).all()
    return got


@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 9, 16, 17, 64])            # every lane group: G = 1, 2, 4, 8, 16, 16, 32, 64
def test_kernel_against_fp64(K, M):
    got = _check_against_fp64(case_logits(K, M))
    if K == 1:
        assert (got["conf"] == 1).all() and (got["entropy"] == 0).all() and (got["labels"] == 0).all()
        assert (got["probs"] == 1).all() and (got["disagree"] == 0).all()
    if M == 1:
        assert (got["disagree"] == 0).all()


def test_member_stride_larger_than_a_member():
    z = case_logits(9, 2)
    got = _check_against_fp64(z, stride_pad=52, tag="stride")
    plain = _run(z)
    for k in got:
        assert got[k].tobytes() == plain[k].tobytes(), k


def test_unequal_weights():
    z = case_logits(9, 2)
    got = _check_against_fp64(z, weights=(3, 1), tag="weights (3, 1)")
    assert not np.array_equal(got["probs"], _run(z)["probs"])
    assert list(normalised_weights((3, 1), 2)) == [0.75, 0.25]
    # a weight of zero takes its member out of p (its own label still counts in the disagreement)
    alone = _run(z[:1])
    zero = _run(z, weights=(1, 0))
    assert zero["probs"].tobytes() == alone["probs"].tobytes() and np.array_equal(zero["labels"], alone["labels"])


# ------------------------------------------------------------------ the exact rules, bit for bit
def test_equal_tops_give_the_lower_index():
    rng = np.random.default_rng(5)
    for K, M in ((9, 2), (17, 4), (64, 1), (2, 2)):
        n = 301
        z = rng.standard_normal((M, n, K)).astype(np.float32)
        a = rng.integers(0, K, n)
        b = (a + 1 + rng.integers(0, K - 1, n)) % K
        top = (5.0 + rng.integers(0, 4, (M, n))).astype(np.float32)      # each member its own value, on the same two classes
        for m in range(M):
            z[m, np.arange(n), a] = top[m]
            z[m, np.arange(n), b] = top[m]
        got = _run(z)
        assert np.array_equal(got["labels"], np.minimum(a, b)), (K, M)
        assert (got["disagree"] == 0).all()
        assert np.array_equal(got["probs"][np.arange(n), a].view(np.uint32), got["probs"][np.arange(n), b].view(np.uint32))


def test_nan_minus_inf_and_large_logits():
    rng = np.random.default_rng(6)
    K, M, n = 9, 2, 130
    z = (4.0 * rng.standard_normal((M, n, K))).astype(np.float32)
    z[1, 3, 4] = np.nan                        # a NaN in ONE member
    z[0, 7, 0] = np.inf                        # a +inf is a NaN row too (inf - inf), as in torch.softmax
    z[:, 11, :] = -np.inf; z[:, 11, 6] = 1.5   # one class left
    z[:, 12, 2:] = -np.inf                     # two classes left
    z[:, 13, :] = -80.0; z[0, 13, 1] = 80.0; z[1, 13, 8] = 80.0
    z[:, 14, :] = 80.0
    got = _run(z)
    for row in (3, 7):
        assert got["labels"][row] == 0 and np.isnan(got["conf"][row]) and np.isnan(got["entropy"][row])
        assert np.isnan(got["probs"][row]).all()
    ref = ensemble_fp64(z)
    assert np.array_equal(got["disagree"][[3, 7]], ref["disagree"][[3, 7]])       # (a NaN member's own label is 0 too)
    ok = np.ones(n, bool); ok[[3, 7]] = False
    assert np.isfinite(got["probs"][ok]).all() and np.isfinite(got["entropy"][ok]).all() and np.isfinite(got["conf"][ok]).all()
    assert got["labels"][11] == 6 and got["conf"][11] == 1.0 and got["entropy"][11] == 0.0
    assert (np.delete(got["probs"][11], 6) == 0).all()
    assert (got["probs"][12, 2:] == 0).all() and 0 < got["entropy"][12] <= np.float32(np.log(2.0)) * (1 + 1e-6)
    assert got["probs"][13, 1] == 0.5 and got["probs"][13, 8] == 0.5 and got["labels"][13] == 1 and got["disagree"][13] == 1
    assert np.abs(got["entropy"][13] - np.log(2.0)) < 1e-6
    assert np.abs(got["probs"][14] - 1.0 / 9).max() < 1e-7 and got["labels"][14] == 0
    assert np.array_equal(got["labels"][[3, 7, 11, 13, 14]], ref["label"][[3, 7, 11, 13, 14]])


def test_two_runs_give_the_same_bytes_and_one_pixel_works():
    z = case_logits(17, 4)
    a, b = _run(z), _run(z)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    one = _run(z[:, 4098:])
    for k in a:
        assert one[k].tobytes() == a[k][4098:].tobytes(), k
    # a pixel's results do not depend on where it lies in the launch
    part = _run(z[:, 1000:1777])
    for k in a:
        assert part[k].tobytes() == a[k][1000:1777].tobytes(), k


def test_only_what_was_asked_for_is_returned():
    from cmlpl_amd.ensemble import ensemble_logits
    zt = torch.from_numpy(case_logits(9, 2, n=64)).to(DEV)
    r = ensemble_logits(zt)
    assert r.probs is None and r.conf is None and r.entropy is None and r.disagree is None and r.labels.shape == (64,)
    full = ensemble_logits(zt, conf=True)
    assert torch.equal(r.labels, full.labels) and full.conf.shape == (64,) and full.probs is None
    one = ensemble_logits(zt[0], probs=True)                       # [n, K]: one member
    assert torch.equal(one.probs, ensemble_logits(zt[:1], probs=True).probs)
    with pytest.raises(ValueError):
        ensemble_logits(zt.transpose(1, 2))


# ------------------------------------------------------------------ composition with the eval forwards
B2 = (103, 11, 11, 103, 9)
W8 = (40, 8, 8, 40, 5)
P = (60, 20, 20, 103, 9)
ASK = dict(probs=True, conf=True, entropy=True, disagree=True)


def _engine(shape):
    from cmlpl_amd import HyperParams, NetShape, TrainEngine
    eng = TrainEngine(NetShape(*shape), 8, 8, HyperParams(), device=DEV, seed=11, hist_rows=8)
    eng.init_params_default(1088)
    return eng


def _scene(shape, rows, cols, seed):
    rng = np.random.default_rng(seed)
    cube = torch.from_numpy(rng.standard_normal((rows, cols, shape[0])).astype(np.float32)).to(DEV)
    X = torch.from_numpy(rng.standard_normal((rows * cols, shape[3])).astype(np.float32)).to(DEV)
    return cube, X


def _same(a, b, what):
    for k in ("labels", "probs", "conf", "entropy", "disagree"):
        assert torch.equal(getattr(a, k).view(torch.int32) if getattr(a, k).dtype == torch.float32 else getattr(a, k),
                           getattr(b, k).view(torch.int32) if getattr(b, k).dtype == torch.float32 else getattr(b, k)), (what, k)


@pytest.fixture(scope="module")
def b2():
    eng = _engine(B2)
    cube, X = _scene(B2, 24, 20, 21)
    return eng, cube, X


@pytest.mark.parametrize("shape", [B2, W8], ids=["B2", "W8"])
def test_pixels_and_cube_are_the_launch_on_the_forwards_logits(shape, b2):
    from cmlpl_amd.ensemble import ensemble_cube, ensemble_logits, ensemble_pixels
    from cmlpl_amd.infer import infer_cube, infer_pixels
    eng, cube, X = b2 if shape == B2 else (_engine(shape),) + _scene(shape, 24, 20, 22)
    n = 24 * 20
    pix = torch.from_numpy(np.random.default_rng(3).permutation(n)[:203].astype(np.int64)).to(DEV)
    _, z = infer_pixels((eng, None), cube, X, pix, spec_rows=pix, want_logits=True)
    want = ensemble_logits(z, **ASK)
    got = ensemble_pixels((eng, None), cube, X, pix, spec_rows=pix, **ASK)
    _same(got, want, "pixels")
    assert got.labels.shape == (203,) and got.probs.shape == (203, shape[4]) and torch.isfinite(got.probs).all()
    _same(ensemble_pixels((eng, None), cube, X, pix, spec_rows=pix, chunk=64, **ASK), want, "pixels in chunks")
    _same(ensemble_pixels([(eng, 0), (eng, 1)], cube, X, pix, spec_rows=pix, **ASK), want, "pixels, one network per entry")
    # the scene: ensemble_cube == ensemble_pixels on arange, in one chunk and in several with a short last one
    every = torch.arange(n, dtype=torch.int64, device=DEV)
    whole = ensemble_pixels((eng, None), cube, X, every, **ASK)
    _same(ensemble_cube((eng, None), cube, X, **ASK), whole, "cube")
    _same(ensemble_cube([(eng, 0), (eng, 1)], cube, X, chunk=200, **ASK), whole, "cube in chunks")
    sub = ensemble_cube((eng, None), cube, X, pixel0=37, n=100, disagree=True)
    assert torch.equal(sub.labels, whole.labels[37:137]) and torch.equal(sub.disagree, whole.disagree[37:137])
    # unequal weights go through, and the members in the order given
    w = ensemble_pixels([(eng, 1), (eng, 0)], cube, X, pix, spec_rows=pix, weights=(1, 3), probs=True)
    assert torch.equal(w.probs, ensemble_logits(z.flip(0).contiguous(), weights=(1, 3), probs=True).probs)
    # one member: its labels are infer_pixels' wherever its logits' top-2 margin is >= 1e-3
    lab0, z0 = infer_cube((eng, 0), cube, X, want_logits=True)
    one = ensemble_cube((eng, 0), cube, X, disagree=True)
    top = torch.topk(z0, 2, dim=1)[0]
    sure = (top[:, 0] - top[:, 1]) >= 1e-3
    print("one member: pixels with a logit margin >= 1e-3: %.4f" % float(sure.float().mean()))
    assert float(sure.float().mean()) >= 0.99
    assert torch.equal(one.labels[sure], lab0[sure]) and int(one.disagree.max()) == 0


def test_by_patches_path():
    """the reference's 20 x 20 windows: the forwards cut their windows on the device, the ensemble is the same launch"""
    from cmlpl_amd.ensemble import ensemble_cube, ensemble_logits, ensemble_pixels
    from cmlpl_amd.infer import infer_fused, infer_pixels
    from cmlpl_amd import NetShape
    assert not infer_fused(NetShape(*P))
    eng = _engine(P)
    cube, X = _scene(P, 24, 20, 23)
    run = torch.arange(100, 164, dtype=torch.int64, device=DEV)               # 64 pixels, as a list and as a range
    _, z = infer_pixels((eng, None), cube, X, run, spec_rows=run, want_logits=True)
    want = ensemble_logits(z, **ASK)
    assert torch.isfinite(want.probs).all()
    _same(ensemble_pixels((eng, None), cube, X, run, spec_rows=run, **ASK), want, "P pixels")
    _same(ensemble_cube((eng, None), cube, X, pixel0=100, n=64, **ASK), want, "P cube")
    _same(ensemble_cube([(eng, 0), (eng, 1)], cube, X, pixel0=100, n=64, chunk=24, **ASK), want, "P cube in chunks")


def test_evaluator_with_the_ensemble(b2):
    from cmlpl_amd import NetShape
    from cmlpl_amd.ensemble import ensemble_pixels
    from cmlpl_amd.evaluate import Evaluator
    eng, cube, X = b2
    K = B2[4]
    rng = np.random.default_rng(4)
    pix = torch.from_numpy(rng.permutation(24 * 20)[:203].astype(np.int64)).to(DEV)
    truth_h = rng.integers(-1, K, 203).astype(np.int64)               # (-1: unlabelled, counted nowhere)
    truth = torch.from_numpy(truth_h).to(DEV)
    ev = Evaluator(NetShape(*B2), cube, X, truth, pix, spec_rows=pix)
    plain = ev.evaluate((eng, None)).cpu().numpy().copy()
    assert ev.logits is None and ev.ens_labels is None and ev.cm_ens is None        # nothing new until it is asked for
    cm = ev.evaluate((eng, None), ensemble=True).cpu().numpy().copy()
    assert cm.shape == (3, K, K) and cm[:2].tobytes() == plain.tobytes()
    lab = ensemble_pixels((eng, None), cube, X, pix, spec_rows=pix).labels.cpu().numpy()
    want = np.zeros((K, K), np.int64)
    keep = truth_h >= 0
    np.add.at(want, (truth_h[keep], lab[keep]), 1)
    assert np.array_equal(cm[2], want) and cm[2].sum() == keep.sum()
    # again, and without: the plain call is what it was, the buffers are re-used
    ptrs = (ev.logits.data_ptr(), ev.ens_labels.data_ptr(), ev.cm_ens.data_ptr())
    assert ev.evaluate((eng, None), ensemble=True).cpu().numpy().tobytes() == cm.tobytes()
    assert ptrs == (ev.logits.data_ptr(), ev.ens_labels.data_ptr(), ev.cm_ens.data_ptr())
    assert ev.evaluate((eng, None)).cpu().numpy().tobytes() == plain.tobytes()
    one = ev.evaluate((eng, 1), ensemble=True).cpu().numpy()
    assert one.shape == (2, K, K) and np.array_equal(one[0], plain[1])


# ------------------------------------------------------------------ the command lines
BASE = ["--synthetic", "B2", "--synthetic_scene", "--num_unlabel", "128", "--labeled_batch_size", "32",
        "--unlabeled_batch_size", "32", "--print_per_batches", "2", "--num_epochs", "2"]


def _cmd(script, *args):
    return subprocess.run([sys.executable, script, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)


def _py(script, *args):
    r = _cmd(script, *args)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ens"))
    f = lambda name: os.path.join(d, name)
    out = _py("train.py", *BASE, "--ensemble", "--eval_every", "1", "--save_eval", f("E.npz"), "--save_loss_hist", f("E.npy"),
              "--save_ckpt", f("E{epoch}.pt"), "--ckpt_every", "1")
    _py("train.py", *BASE, "--no_eval", "--save_loss_hist", f("plain.npy"), "--save_ckpt", f("plain.pt"))
    return dict(dir=d, out=out, f=f)


def test_train_with_the_ensemble(runs):
    from cmlpl_amd import checkpoint
    from tests.test_gpu_ema import PARENT_ARGS, PARENT_EXTRA
    out, f = runs["out"], runs["f"]
    val = [ln for ln in out if re.match(r"^Epoch \d+/2: validation", ln)]
    pat = r"^Epoch %d/2: validation%s OA = \d+\.\d\d AA = \d+\.\d\d Kappa = -?\d+\.\d\d$"
    assert len(val) == 6, val
    for e in range(2):
        for j, tag in enumerate(("", "1", "_ens")):
            assert re.match(pat % (e + 1, tag), val[3 * e + j]), val[3 * e + j]
    assert [ln.split("=")[0] for ln in out if ln.startswith(" OA")] == [" OA", " OA1", " OA_ens"]
    assert sum(ln.startswith("producerA_ens:") for ln in out) == 1 and sum(ln.startswith("AA_ens=") for ln in out) == 1
    best = [ln for ln in out if ln.startswith("best validation")]
    assert len(best) == 3 and re.match(r"^best validation_ens: epoch [12] OA = \d+\.\d\d$", best[2]), best
    # the flag looks at the run and leaves it alone
    assert np.load(f("E.npy")).tobytes() == np.load(f("plain.npy")).tobytes()
    z = np.load(f("E.npz"))
    assert z["curve_ens"].shape == (2, 3) and z["cm_ens"].shape == (2, 9, 9) and list(z["epochs_ens"]) == [1, 2]
    assert z["curve"].shape == (2, 2, 3) and z["cm"].shape == (2, 2, 9, 9)
    assert (z["cm_ens"].sum((1, 2)) == 64 * 64).all()
    from cmlpl_amd.evaluate import metrics
    for i in range(2):
        OA, Kappa, _, AA = metrics(z["cm_ens"][i])
        assert tuple(z["curve_ens"][i]) == (OA, AA, Kappa)
    assert ("%.2f" % (z["curve_ens"][1, 0] * 100)) in val[5]
    # the whole-image ensemble after the run and the last validation count the same pixels of the same networks
    oa_line = [ln for ln in out if ln.startswith(" OA_ens")][0]
    assert oa_line.startswith(" OA_ens=%.2f," % (z["curve_ens"][1, 0] * 100)), (oa_line, z["curve_ens"][1])
    ck, plain = checkpoint.load(f("E2.pt")), checkpoint.load(f("plain.pt"))
    assert set(plain["extra"]) == PARENT_EXTRA and set(plain["extra"]["args"]) == PARENT_ARGS
    assert set(ck["extra"]) == PARENT_EXTRA | {"eval_epochs_ens", "eval_curve_ens", "eval_cms_ens"}
    assert ck["extra"]["args"]["ensemble"] is True and ck["extra"]["eval_epochs_ens"] == [1, 2]
    assert ck["extra"]["eval_curve_ens"].numpy().tobytes() == z["curve_ens"].tobytes()
    assert ck["extra"]["eval_cms_ens"].numpy().tobytes() == z["cm_ens"].tobytes()


def test_resumed_run_reproduces_the_ensembles_curve(runs):
    f = runs["f"]
    out = _py("train.py", *BASE, "--ensemble", "--no_eval", "--eval_every", "1", "--save_eval", f("R.npz"),
              "--save_loss_hist", f("R.npy"), "--resume", f("E1.pt"))
    z, zs = np.load(f("R.npz")), np.load(f("E.npz"))
    for k in ("curve", "epochs", "cm", "curve_ens", "cm_ens", "epochs_ens"):
        assert z[k].tobytes() == zs[k].tobytes() and z[k].shape == zs[k].shape, k
    assert np.load(f("R.npy")).tobytes() == np.load(f("E.npy")).tobytes()
    ens = lambda lines: [ln for ln in lines if "validation_ens" in ln]
    assert ens(out) == ens(runs["out"])[1:] and len(ens(out)) == 2        # (epoch 2's line and the best line)


def test_predict_ensemble_outputs(runs):
    f = runs["f"]
    n, K = 64 * 64, 9
    got = _py("predict.py", "--ckpt", f("E2.pt"), "--synthetic", "B2", "--net", "ensemble", "--out", f("lab.npy"),
              "--proba", f("p.npy"), "--confidence", f("c.npy"), "--entropy", f("e.npy"))
    lab, p, c, e = (np.load(f(x)) for x in ("lab.npy", "p.npy", "c.npy", "e.npy"))
    assert lab.shape == (n,) and lab.dtype == np.int64 and p.shape == (n, K) and p.dtype == np.float32
    assert c.shape == (n,) and c.dtype == np.float32 and e.shape == (n,) and e.dtype == np.float32
    # rows sum to 1: every p_c is within 6 x 2^-24 relative (expf one ulp, the division, the four additions of the
    # butterfly denominator, the weighted sum), so the fp64 row sum is within 6 x 2^-24 of 1; allowed 2 K x 2^-24
    assert np.abs(p.astype(np.float64).sum(1) - 1).max() <= 2 * K * 2.0 ** -24
    sure = top2_margin(p.astype(np.float64)) >= MARGIN
    assert sure.mean() >= 0.99 and np.array_equal(p.argmax(1)[sure], lab[sure])
    assert np.array_equal(first_max(p), lab) and np.array_equal(p.max(1), c)          # (the kernel's own p: exactly)
    assert (e >= 0).all() and (e <= np.log(K) * (1 + 1e-6)).all() and (c >= 1.0 / K - 1e-7).all() and (c <= 1).all()
    # the same lines as the run's own third block
    want = [ln for ln in runs["out"] if ln.startswith(" OA_ens")]
    assert [ln for ln in got if ln.startswith(" OA")] == want
    # a file without teachers
    r = _cmd("predict.py", "--ckpt", f("E2.pt"), "--synthetic", "B2", "--net", "ensemble_all")
    assert r.returncode != 0 and "--ema" in r.stderr and "Teacher" in r.stderr


def test_predict_one_network_with_its_own_softmax(runs):
    """a single --net: the label map stays infer_cube's argmax of the logits, the new files are its own softmax"""
    from cmlpl_amd import checkpoint
    from cmlpl_amd.infer import infer_cube
    from cmlpl_amd.models import BaseNet2
    from hsi_loader import SyntheticScene
    f = runs["f"]
    n, K = 64 * 64, 9
    _py("predict.py", "--ckpt", f("E2.pt"), "--synthetic", "B2", "--net", "1", "--out", f("lab1.npy"), "--proba", f("p1.npy"),
        "--entropy", f("e1.npy"))
    lab1, p1 = np.load(f("lab1.npy")), np.load(f("p1.npy"))
    assert p1.shape == (n, K) and np.load(f("e1.npy")).shape == (n,) and not os.path.exists(f("c1.npy"))
    mod = BaseNet2(num_features=B2[3], dropout=0.8, num_classes=K, in_channels=B2[0], window=B2[1]).to(DEV)
    mod.load_state_dict(checkpoint.load(f("E2.pt"))["Base1"])
    src = SyntheticScene(B2, 64, 64, seed=3).cube_source(torch.device(DEV))
    want, z = infer_cube(mod.eval(), src.cube, src.spectra, want_logits=True)
    assert np.array_equal(lab1, want.cpu().numpy())
    top = torch.topk(z, 2, dim=1)[0]
    sure = ((top[:, 0] - top[:, 1]) >= 1e-3).cpu().numpy()
    assert sure.mean() >= 0.99 and np.array_equal(p1.argmax(1)[sure], lab1[sure])
    ref = torch.softmax(z.double(), 1).cpu().numpy()
    assert np.abs(p1 - ref).max() <= 8 * np.abs(torch.softmax(z.cpu(), 1).numpy() - ref).max()
