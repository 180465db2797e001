"""GPU: test-time augmentation against its definition (include/cmlpl.h, "THE DEFINITION OF A VIEW"; restated in numpy in
tests/test_tta_host.py).

  1. cmlpl_tta_patches forms the documented generator (2e-5 absolute: the project's tolerance for the hardware's
     log2 / sin / cos against numpy's, tests/test_gpu_step.py).
  2. The fused noisy forward (cmlpl_infer_cube_tta) sees exactly those views: its logits against this library's general
     eval forward on ``views_of`` (1e-5 relative + 1e-5 max |z|, the bound of test_infer_cube_equals_the_patch_path) and
     against the fp64 oracle on the downloaded views (1e-4 max |z| + 1e-5, test_infer_cube_matches_the_oracle's).
  3. What a view must not depend on, bit for bit.
  4. cmlpl_ensemble_views: cmlpl_ensemble's bytes at one view; the fp64 definition beyond, with tests/test_gpu_ensemble.py's
     yardstick (8 x the error of the same arithmetic in fp32 torch on the CPU; labels and disagreement exact where the
     fp64 margins are >= 1e-5, which may leave out at most 1 % of a case).
  5. The host functions and the two command lines."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV, report
from tests.test_ensemble_host import case_logits, top2_margin
from tests.test_gpu_ensemble import ASK, _engine, _same
from tests.test_gpu_infer import _module, _scene
from tests.test_tta_host import (VIEW_CASES, ensemble_views_fp32_torch, ensemble_views_fp64, view_spectrum_noise,
                                 view_window_noise, views_case)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-5
B2 = (103, 11, 11, 103, 9)
B5 = (48, 15, 15, 48, 20)
P = (60, 20, 20, 103, 9)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _eq(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ 1. the generator
@pytest.mark.parametrize("t", [0, 3])
@pytest.mark.parametrize("C,w,bands", [(103, 11, 103), (30, 8, 30)])
def test_tta_patches_form_the_documented_generator(C, w, bands, t):
    from cmlpl_amd.tta import TTA, views_of
    rows, cols = 14, 17
    cube = torch.zeros(rows, cols, C, device=DEV)
    X = torch.zeros(rows * cols, bands, device=DEV)
    # corners, edges, the interior, a repeated entry
    pix_h = [0, cols - 1, (rows - 1) * cols, rows * cols - 1, 5, 3 * cols, 6 * cols + 8, 4 * cols + cols - 1, 6 * cols + 8, 5]
    pix = torch.tensor(pix_h, dtype=torch.int64, device=DEV)
    xp, x = views_of(cube, X, pix, w, TTA(4, 1.0, seed=1088), t)
    assert xp.shape == (len(pix_h), C, w, w) and x.shape == (len(pix_h), bands)
    want_p = np.stack([view_window_noise(1088, t, Pn, C, w) for Pn in pix_h])
    want_x = np.stack([view_spectrum_noise(1088, t, Pn, bands) for Pn in pix_h])
    ep = np.abs(xp.cpu().numpy() - want_p).max()
    ex = np.abs(x.cpu().numpy() - want_x).max()
    print("C %d w %d t %d: windows max |err| %.2e, spectra %.2e (allowed 2e-5)" % (C, w, t, ep, ex))
    assert ep <= 2e-5 and ex <= 2e-5
    assert _eq(xp[6], xp[8]) and _eq(x[6], x[8]) and _eq(xp[4], xp[9])          # a view belongs to the pixel, not to the entry
    assert not _eq(xp[6], xp[4])
    # sigma scales it, and compact spectra rows take the pixel's view all the same
    xp2, x2 = views_of(cube, X[:len(pix_h)].contiguous(), pix, w, TTA(4, 0.25, seed=1088), t,
                       spec_rows=torch.arange(len(pix_h), device=DEV))
    assert np.abs(xp2.cpu().numpy() - 0.25 * want_p).max() <= 5e-6 and np.abs(x2.cpu().numpy() - 0.25 * want_x).max() <= 5e-6


def test_the_clean_view_is_extract_patches_and_noise_is_added_with_one_fma():
    from cmlpl_amd.patches import extract_patches
    from cmlpl_amd.tta import TTA, views_of
    rows, cols, C, w = 9, 12, 30, 8
    cube_h, X_h = _scene(rows, cols, C, 30, 7)
    cube, X = torch.from_numpy(cube_h).to(DEV), torch.from_numpy(X_h).to(DEV)
    pix = torch.arange(rows * cols, dtype=torch.int64, device=DEV)                # every pixel: every mirrored border
    clean = extract_patches(cube, pix, w)
    tta = TTA(2, 0.5, seed=99)
    xp0, x0 = views_of(cube, X, pix, w, tta, None)
    assert _eq(xp0, clean) and _eq(x0, X)
    xp, x = views_of(cube, X, pix, w, tta, 1)
    zero = views_of(torch.zeros_like(cube), torch.zeros_like(X), pix, w, TTA(2, 1.0, seed=99), 1)
    # fmaf(z, sigma, x) with sigma = 0.5: z / 2 is exact, so the fused product-sum is the rounded sum
    assert _eq(xp, zero[0] * 0.5 + clean) and _eq(x, zero[1] * 0.5 + X)
    assert torch.isfinite(xp).all()


# ------------------------------------------------------------------ 2. the fused noisy forward
CASES = [("B2", B2, 20, 24, True), ("B4", (200, 11, 11, 200, 16), 12, 14, False), ("B5", B5, 16, 18, True),
         ("W10", (17, 10, 10, 17, 7), 13, 18, False), ("P", P, 22, 26, False)]


@pytest.mark.parametrize("name,shape,rows,cols,oracle", CASES, ids=[c[0] for c in CASES])
def test_noisy_forward_sees_exactly_the_views(name, shape, rows, cols, oracle):
    from cmlpl_amd.infer import infer_cube, infer_fused
    from cmlpl_amd.tta import TTA, infer_cube_view, views_of
    s = O.NetShape(*shape)
    assert infer_fused(s) == (name != "P")
    cube_h, X_h = _scene(rows, cols, s.C, s.bands, 99)
    dc, dx = torch.from_numpy(cube_h).to(DEV), torch.from_numpy(X_h).to(DEV)
    net, p = _module(s, 61, scale=8.0)
    tta, t = TTA(3, 0.5, seed=1088), 2
    labels, logits = infer_cube_view(net, dc, dx, tta, t, chunk=1000)
    pix = torch.arange(rows * cols, dtype=torch.int64, device=DEV)
    XP, XS = views_of(dc, dx, pix, s.H, tta, t)
    with torch.no_grad():
        z, _ = net(XP, XS)
    zmax = float(z.abs().max())
    report(f"[{name}] logits, fused noisy forward vs the general forward on views_of", logits, z, 1e-5, 1e-5 * zmax)
    top2 = z.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-4 * zmax
    assert int(sure.sum()) > 0.9 * len(sure)
    assert torch.equal(labels[sure], z.argmax(1)[sure])
    clean = infer_cube(net, dc, dx, want_logits=True)[1]
    assert float((logits - clean).abs().max()) > 1e-3 * zmax                  # the view is not the clean window
    if oracle:
        with torch.no_grad():
            want, _ = O.basenet2_forward(p, XP.cpu(), XS.cpu(), None)
        report(f"[{name}] logits vs the fp64 oracle on the downloaded views", logits, want, 0.0,
               1e-4 * float(want.abs().max()) + 1e-5)


# ------------------------------------------------------------------ 3. invariances, bit for bit
@pytest.fixture(scope="module", params=[("B2", B2, 20, 24), ("B5", B5, 16, 18)], ids=["B2", "B5"])
def scene(request):
    from cmlpl_amd.tta import TTA, infer_cube_view
    name, shape, rows, cols = request.param
    s = O.NetShape(*shape)
    cube_h, X_h = _scene(rows, cols, s.C, s.bands, 31)
    dc, dx = torch.from_numpy(cube_h).to(DEV), torch.from_numpy(X_h).to(DEV)
    nets = (_module(s, 61, scale=8.0)[0], _module(s, 62, scale=8.0)[0])
    tta = TTA(3, 0.5, seed=5)
    whole = [infer_cube_view(n, dc, dx, tta, 1) for n in nets]                # (labels, logits) of view 1, computed once
    return dict(s=s, n=rows * cols, cube=dc, X=dx, nets=nets, tta=tta, whole=whole)


def test_list_fed_equals_range_fed_in_any_order_with_repeats_and_compact_rows(scene):
    from cmlpl_amd.tta import infer_pixels_view
    c = scene
    rng = np.random.default_rng(3)
    pix_h = np.concatenate([rng.permutation(c["n"])[:150], [7, 7, 0, c["n"] - 1, 7]]).astype(np.int64)
    pix = torch.from_numpy(pix_h).to(DEV)
    lab_w, z_w = c["whole"][0]
    lab, z = infer_pixels_view(c["nets"][0], c["cube"], c["X"], pix, c["tta"], 1, spec_rows=pix)
    assert _eq(z, z_w[pix]) and torch.equal(lab, lab_w[pix])
    compact = c["X"][pix].contiguous()                                        # a split's rows: item i's spectrum is row i
    lab_c, z_c = infer_pixels_view(c["nets"][0], c["cube"], compact, pix, c["tta"], 1)
    assert _eq(z_c, z_w[pix]) and torch.equal(lab_c, lab_w[pix])
    lab_k, z_k = infer_pixels_view(c["nets"][0], c["cube"], compact, pix, c["tta"], 1, chunk=64)
    assert _eq(z_k, z_w[pix]) and torch.equal(lab_k, lab_w[pix])
    # two networks in one launch chain == two single calls: both score the same views
    lab2, z2 = infer_pixels_view(c["nets"], c["cube"], c["X"], pix, c["tta"], 1, spec_rows=pix)
    assert z2.shape == (2, len(pix_h), c["s"].K)
    for k in range(2):
        assert _eq(z2[k], c["whole"][k][1][pix]) and torch.equal(lab2[k], c["whole"][k][0][pix]), k
    assert not _eq(z2[0], z2[1])


def test_chunks_subranges_runs_and_sigma_zero(scene):
    from cmlpl_amd.infer import infer_cube
    from cmlpl_amd.tta import TTA, infer_cube_view
    c = scene
    net, n = c["nets"][0], c["n"]
    lab_w, z_w = c["whole"][0]
    for chunk in (8, 1000):
        lab, z = infer_cube_view(net, c["cube"], c["X"], c["tta"], 1, chunk=chunk)
        assert _eq(z, z_w) and torch.equal(lab, lab_w), chunk
    lab, z = infer_cube_view(net, c["cube"], c["X"], c["tta"], 1)             # again: the same bytes
    assert _eq(z, z_w) and torch.equal(lab, lab_w)
    lab, z = infer_cube_view(net, c["cube"], c["X"], c["tta"], 1, pixel0=5, n=n - 16)     # off the 8-pixel dealing
    assert _eq(z, z_w[5:n - 11]) and torch.equal(lab, lab_w[5:n - 11])
    lab_c, z_c = infer_cube(net, c["cube"], c["X"], want_logits=True)
    for tta, t in ((TTA(3, 0.0, seed=5), 1), (c["tta"], None)):               # sigma 0, and the clean block
        lab, z = infer_cube_view(net, c["cube"], c["X"], tta, t)
        assert _eq(z, z_c) and torch.equal(lab, lab_c)
    assert not _eq(z_w, z_c)
    other = infer_cube_view(net, c["cube"], c["X"], c["tta"], 2)[1]           # another view, another seed: other logits
    seed = infer_cube_view(net, c["cube"], c["X"], TTA(3, 0.5, seed=6), 1)[1]
    assert not _eq(other, z_w) and not _eq(seed, z_w)


# ------------------------------------------------------------------ 4. cmlpl_ensemble_views
def _views_run(z, weights=None, pad=0):
    """the kernel on logits [M, V, n, K] (numpy): every output as numpy; pad: floats between the blocks"""
    from cmlpl_amd.tta import ensemble_views_logits
    M, V, n, K = z.shape
    if pad:
        buf = torch.full((M, V, n * K + pad), float("nan"), dtype=torch.float32, device=DEV)
        buf[:, :, :n * K] = torch.from_numpy(z.reshape(M, V, n * K)).to(DEV)
        zt = buf.as_strided((M, V, n, K), (V * (n * K + pad), n * K + pad, K, 1))
    else:
        zt = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
    r = ensemble_views_logits(zt, weights=weights, **ASK)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("K", [2, 9, 16, 20])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_one_view_is_cmlpl_ensemble_bit_for_bit(K, M):
    from cmlpl_amd.ensemble import ensemble_logits
    z = case_logits(K, M, n=1031)
    zt = torch.from_numpy(z).to(DEV)
    for weights in (None, tuple(range(1, M + 1))):
        want = ensemble_logits(zt, weights=weights, **ASK)
        _same(_views_run(z[:, None], weights), want, ("contiguous", K, M, weights))
        _same(_views_run(z[:, None], weights, pad=52), want, ("padded strides", K, M, weights))
        # the members as VIEWS of one member, strides swapped: the same sum in the same order when the weights are equal
        if weights is None:
            from cmlpl_amd.tta import ensemble_views_logits
            r = ensemble_views_logits(zt[None], **ASK)
            assert torch.equal(r.labels, want.labels) and torch.equal(r.disagree, want.disagree)


@pytest.mark.parametrize("K,M,V", VIEW_CASES, ids=["K%d-M%d-V%d" % c for c in VIEW_CASES])
def test_views_kernel_against_fp64(K, M, V):
    z = views_case(K, M, V)
    weights = None if M == 1 else tuple(range(1, M + 1))
    for w in (None, weights) if weights else (None,):
        ref = ensemble_views_fp64(z, w)
        p32, e32 = ensemble_views_fp32_torch(z, w)
        tol_p = 8 * np.abs(p32 - ref["p"]).max()
        tol_e = 8 * np.abs(e32 - ref["entropy"]).max()
        r = _views_run(z, w)
        got = {k: getattr(r, k).cpu().numpy() for k in ("labels", "probs", "conf", "entropy", "disagree")}
        err_p = np.abs(got["probs"] - ref["p"]).max()
        err_c = np.abs(got["conf"] - ref["conf"]).max()
        err_e = np.abs(got["entropy"] - ref["entropy"]).max()
        sure = top2_margin(ref["p"]) >= MARGIN
        sure_m = sure & (top2_margin(ref["pm"]) >= MARGIN).all((0, 1))
        print("K %d M %d V %d weights %s: p err %.2e (allowed %.2e) conf err %.2e entropy err %.2e (allowed %.2e) under the "
              "margin %.4f" % (K, M, V, w, err_p, tol_p, err_c, err_e, tol_e, 1 - sure.mean()))
        assert err_p <= tol_p and err_c <= tol_p and err_e <= tol_e
        assert sure.mean() >= 0.99
        assert np.array_equal(got["labels"][sure], ref["label"][sure])
        assert np.array_equal(got["disagree"][sure_m], ref["disagree"][sure_m])
        assert ((got["labels"] >= 0) & (got["labels"] < K)).all()
        assert ((got["disagree"] >= 0) & (got["disagree"] <= M * V)).all()
    again = _views_run(z, None)
    _same(again, _views_run(z, None), "two runs")
    part = _views_run(np.ascontiguousarray(z[:, :, 1000:1777]), None)             # a pixel's results do not depend on its place
    for k in ("labels", "probs", "conf", "entropy", "disagree"):
        assert _eq(getattr(part, k), getattr(again, k)[1000:1777]), k


def test_nan_inf_and_ties_over_several_views():
    rng = np.random.default_rng(6)
    K, M, V, n = 9, 2, 3, 130
    z = (4.0 * rng.standard_normal((M, V, n, K))).astype(np.float32)
    z[1, 2, 3, 4] = np.nan                     # a NaN in ONE block
    z[0, 1, 7, 0] = np.inf                     # a +inf is a NaN row too (inf - inf), as in torch.softmax
    z[:, :, 11, :] = -np.inf; z[:, :, 11, 6] = 1.5
    z[:, :, 12, 2:] = -np.inf
    z[:, :, 13, :] = -80.0; z[0, :, 13, 1] = 80.0; z[1, :, 13, 8] = 80.0       # the members disagree, their views agree
    z[:, :, 14, :] = 80.0
    z[:, :, 15, :] = 0.0; z[:, :, 15, 2] = 50.0; z[:, :, 15, 6] = 50.0          # two equal tops in every block
    r = _views_run(z)
    got = {k: getattr(r, k).cpu().numpy() for k in ("labels", "probs", "conf", "entropy", "disagree")}
    ref = ensemble_views_fp64(z)
    for row in (3, 7):
        assert got["labels"][row] == 0 and np.isnan(got["conf"][row]) and np.isnan(got["entropy"][row])
        assert np.isnan(got["probs"][row]).all()
    assert np.array_equal(got["disagree"][[3, 7]], ref["disagree"][[3, 7]])
    ok = np.ones(n, bool); ok[[3, 7]] = False
    assert np.isfinite(got["probs"][ok]).all() and np.isfinite(got["entropy"][ok]).all() and np.isfinite(got["conf"][ok]).all()
    assert got["labels"][11] == 6 and got["entropy"][11] == 0.0 and (np.delete(got["probs"][11], 6) == 0).all()
    assert abs(got["conf"][11] - 1.0) <= 6 * 2.0 ** -24                      # (six fp32 weights of 1 / 6)
    assert (got["probs"][12, 2:] == 0).all() and 0 < got["entropy"][12] <= np.float32(np.log(2.0)) * (1 + 1e-6)
    assert got["probs"][13, 1] == got["probs"][13, 8] and got["labels"][13] == 1 and got["disagree"][13] == 3
    assert abs(got["probs"][13, 1] - 0.5) <= 3 * 2.0 ** -24 and np.abs(got["entropy"][13] - np.log(2.0)) < 1e-6
    assert np.abs(got["probs"][14] - 1.0 / 9).max() < 1e-6 and got["labels"][14] == 0
    assert got["labels"][15] == 2 and got["disagree"][15] == 0
    assert got["probs"][15, 2].view(np.uint32) == got["probs"][15, 6].view(np.uint32)
    assert np.array_equal(got["labels"][[3, 7, 11, 13, 14, 15]], ref["label"][[3, 7, 11, 13, 14, 15]])


def test_argument_errors_come_back_before_a_launch_on_a_device_too():
    from tests import test_tta_host as H
    H.test_ensemble_views_argument_checks_return_e_arg_before_any_launch()
    H.test_view_entry_points_refuse_bad_arguments_before_any_launch()
    torch.cuda.synchronize()                                                  # nothing was launched: nothing can have faulted


# ------------------------------------------------------------------ 5. end to end
def _by_hand(eng, cube, X, tta, pixel0=0, n=None):
    from cmlpl_amd.tta import ensemble_views_logits, infer_cube_view
    z = torch.stack([torch.stack([infer_cube_view((eng, k), cube, X, tta, t, pixel0=pixel0, n=n)[1] for t in tta.blocks()])
                     for k in range(2)])
    return ensemble_views_logits(z, **ASK), z


def test_tta_cube_and_pixels_are_the_views_launch_on_the_forwards_logits():
    from cmlpl_amd.tta import TTA, tta_cube, tta_pixels
    eng = _engine(B2)
    cube_h, X_h = _scene(20, 24, B2[0], B2[3], 21)
    cube, X = torch.from_numpy(cube_h).to(DEV), torch.from_numpy(X_h).to(DEV)
    tta = TTA(3, 0.5, seed=1088)
    want, z = _by_hand(eng, cube, X, tta)
    assert z.shape == (2, 4, 480, 9) and torch.isfinite(want.probs).all()
    _same(tta_cube((eng, None), cube, X, tta, **ASK), want, "cube")
    _same(tta_cube([(eng, 0), (eng, 1)], cube, X, tta, chunk=200, **ASK), want, "cube in chunks, one network per entry")
    every = torch.arange(480, dtype=torch.int64, device=DEV)
    _same(tta_pixels((eng, None), cube, X, every, tta, spec_rows=every, **ASK), want, "pixels")
    _same(tta_pixels((eng, None), cube, X, every, tta, chunk=64, **ASK), want, "pixels, compact rows, in chunks")
    sub = tta_cube((eng, None), cube, X, tta, pixel0=37, n=100, disagree=True)
    assert torch.equal(sub.labels, want.labels[37:137]) and torch.equal(sub.disagree, want.disagree[37:137])
    assert sub.probs is None and sub.conf is None
    # without the clean block, weighted, one member
    noisy = TTA(3, 0.5, seed=1088, clean=False)
    from cmlpl_amd.tta import ensemble_views_logits
    w = tta_cube((eng, None), cube, X, noisy, weights=(1, 3), probs=True)
    assert _eq(w.probs, ensemble_views_logits(z[:, 1:], weights=(1, 3), probs=True).probs)
    one = tta_cube((eng, 1), cube, X, tta, **ASK)
    _same(one, ensemble_views_logits(z[1:], **ASK), "one member")
    assert int(want.disagree.max()) <= 8


def test_tta_by_patches():
    """the reference's 20 x 20 windows: the views are cut on the device (cmlpl_tta_patches), the reduction is the same launch"""
    from cmlpl_amd.tta import TTA, tta_cube, tta_pixels
    eng = _engine(P)
    cube_h, X_h = _scene(24, 20, P[0], P[3], 23)
    cube, X = torch.from_numpy(cube_h).to(DEV), torch.from_numpy(X_h).to(DEV)
    tta = TTA(2, 0.5, seed=3)
    want, _ = _by_hand(eng, cube, X, tta, pixel0=100, n=64)
    assert torch.isfinite(want.probs).all()
    run = torch.arange(100, 164, dtype=torch.int64, device=DEV)
    _same(tta_cube((eng, None), cube, X, tta, pixel0=100, n=64, **ASK), want, "P cube")
    _same(tta_cube([(eng, 0), (eng, 1)], cube, X, tta, pixel0=100, n=64, chunk=24, **ASK), want, "P cube in chunks")
    _same(tta_pixels((eng, None), cube, X, run, tta, spec_rows=run, **ASK), want, "P pixels")


W8_RUN = ["--synthetic", "W8", "--synthetic_scene", "--num_unlabel", "128", "--labeled_batch_size", "32",
          "--unlabeled_batch_size", "32", "--print_per_batches", "2", "--num_epochs", "1"]


def _py(script, *args):
    r = subprocess.run([sys.executable, script, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tta"))
    f = lambda name: os.path.join(d, name)
    out = _py("train.py", *W8_RUN, "--tta", "--m", "2", "--save_loss_hist", f("T.npy"), "--save_ckpt", f("T.pt"))
    plain = _py("train.py", *W8_RUN, "--save_loss_hist", f("plain.npy"))
    return dict(out=out, plain=plain, f=f)


def _stable(lines):
    """a run's printed lines without the ones that carry a wall time"""
    return [ln for ln in lines if not re.search(r"\d s\b| s \(|ms/step|time ==|ready in", ln)]


def test_train_with_tta_adds_one_result_block_and_leaves_the_run_alone(runs):
    out, plain, f = runs["out"], runs["plain"], runs["f"]
    assert [ln.split("=")[0] for ln in out if ln.startswith(" OA")] == [" OA", " OA1", " OA_tta"]
    assert sum(ln.startswith("producerA_tta:") for ln in out) == 1 and sum(ln.startswith("AA_tta=") for ln in out) == 1
    assert sum("tta inference time ==" in ln and "2 networks x 2 views + the clean window, noise 0.5" in ln for ln in out) == 1
    assert np.load(f("T.npy")).tobytes() == np.load(f("plain.npy")).tobytes()
    assert not any("_tta" in ln or "tta " in ln for ln in plain)
    i = next(k for k, ln in enumerate(out) if ln.startswith("tta inference time"))
    # the lines of the run without the flag, in their order, then the new block and nothing else
    assert _stable(out[:i]) == _stable(plain) and len(out) - i <= 12


def test_predict_tta(runs):
    from cmlpl_amd import checkpoint
    from cmlpl_amd.infer import infer_cube
    from cmlpl_amd.models import BaseNet2
    from cmlpl_amd.tta import TTA, tta_cube
    from hsi_loader import SyntheticScene
    import train
    f = runs["f"]
    W8 = train.SYNTH["W8"]
    n, K = 64 * 64, W8[4]
    got = _py("predict.py", "--ckpt", f("T.pt"), "--synthetic", "W8", "--net", "ensemble", "--tta", "3", "--out", f("lab.npy"),
              "--proba", f("p.npy"), "--confidence", f("c.npy"), "--entropy", f("e.npy"))
    lab, p, c, e = (np.load(f(x)) for x in ("lab.npy", "p.npy", "c.npy", "e.npy"))
    assert lab.shape == (n,) and lab.dtype == np.int64 and p.shape == (n, K) and p.dtype == np.float32
    assert c.shape == (n,) and c.dtype == np.float32 and e.shape == (n,) and e.dtype == np.float32
    assert [ln.split("=")[0] for ln in got if ln.startswith(" OA")] == [" OA_tta"]
    assert sum(ln.startswith("producerA_tta:") for ln in got) == 1 and sum(ln.startswith("AA_tta=") for ln in got) == 1
    ck = checkpoint.load(f("T.pt"))
    mods = []
    for key in ("Base", "Base1"):
        mod = BaseNet2(num_features=W8[3], dropout=0.8, num_classes=K, in_channels=W8[0], window=W8[1]).to(DEV)
        mod.load_state_dict(ck[key])
        mods.append(mod.eval())
    src = SyntheticScene(W8, 64, 64, seed=3).cube_source(torch.device(DEV))
    want = tta_cube(mods, src.cube, src.spectra, TTA(3, ck["identity"]["hp"]["noise"]), probs=True, conf=True, entropy=True)
    assert np.array_equal(lab, want.labels.cpu().numpy())
    for a, b in ((p, want.probs), (c, want.conf), (e, want.entropy)):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    # one network, the noisy views alone, another noise and seed
    _py("predict.py", "--ckpt", f("T.pt"), "--synthetic", "W8", "--net", "1", "--tta", "2", "--tta_noise", "0.25", "--tta_seed", "7",
        "--tta_no_clean", "--out", f("lab1.npy"), "--confidence", f("c1.npy"))
    one = tta_cube(mods[1], src.cube, src.spectra, TTA(2, 0.25, seed=7, clean=False), conf=True)
    assert np.array_equal(np.load(f("lab1.npy")), one.labels.cpu().numpy())
    assert np.load(f("c1.npy")).tobytes() == one.conf.cpu().numpy().tobytes()
    # without --tta: what it wrote before -- infer_cube's argmax, the untagged lines
    plain = _py("predict.py", "--ckpt", f("T.pt"), "--synthetic", "W8", "--net", "0", "--out", f("lab0.npy"))
    assert np.array_equal(np.load(f("lab0.npy")), infer_cube(mods[0], src.cube, src.spectra).cpu().numpy())
    assert [ln.split("=")[0] for ln in plain if ln.startswith(" OA")] == [" OA"] and not any("tta" in ln for ln in plain)
    assert [ln for ln in plain if ln.startswith(" OA")] == [ln for ln in runs["out"] if ln.startswith(" OA=")]
