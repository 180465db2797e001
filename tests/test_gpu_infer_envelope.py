"""GPU: every route and edge of whole-scene inference against the fp64 oracle (tests/infer_cases.py; the routing itself
is held to the same table without a device by tests/test_infer_route_cpu.py).

`infer_cube`, `infer_pixels` and their views are what predict.py, Evaluator, the ensemble and TTA stand on.  The window
gather of the fused forward (conv3_stage's CUBE branches in csrc/conv3x3.hip) walks the band chunks with code of its
own -- clamped per-element loads, transposed LDS stores, the view's noise index -- and each case of the table is there
for ONE regime of that walk, of the scene's mirror folds, or of the by-patches route, and says which.

Per case the reference is the oracle's extract_patches -> basenet2_forward in FLOAT64, eval mode, over every pixel of the
scene.  No ReLU gates: the eval forward is continuous in its pre-activations, so a decision that rounding flips costs no
more than the rounding that flipped it.  The logits must lie within BOUND = 2e-6 of the largest reference logit -- the
bound the same arithmetic meets in training (tests/test_gpu_shape_envelope.py); the fp32 oracle's own distance is printed
next to the device's, and a case whose fp32 oracle is itself beyond the bound would get 4 x the oracle's measured error
(docs/EXPERIMENTS.md, "Inference envelope" -- none needs it).  The labels must be `_first_max` of the device's own logits
on EVERY pixel, and the oracle's argmax wherever its top-two margin exceeds 4 BOUND max|z| (at most 2 % of a case's
pixels may be left out this way).

Then what a prediction must not depend on, bit for bit (the feed: ranges, chunks, lists in any order with repeats, two
networks in one call), the views of test-time augmentation on the shapes where the noise index runs a second and a
third pass, the fused cases forced through the by-patches route, the device's argmax rule on ties and NaNs, and the
refusals -- a scene smaller than half a window, a window no cut takes -- before any launch."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV
from tests.infer_cases import (ARGMAX_CASES, BY_ID, CASES, CUT_TOO_LARGE, FORCED_BY_PATCHES, FORCED_REFUSED, FUSED4,
                               FUSED8, PATCHES, VIEW_CASES, VIEW_NO_CUT)
from tests.test_gpu_shape_envelope import BOUND, _launch_counts
from tests.test_spatial_host import apply_element

pytestmark = pytest.mark.gpu
FUSED = [c for c in CASES if c.fused]
SCALE = 8.0                   # the classifier weight's factor (tests/test_gpu_infer.py): logits of a few units


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _eq(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@contextlib.contextmanager
def _switches(env):
    """CMLPL_* switches for the library calls inside; the environment and the library's table are restored"""
    from cmlpl_amd import _lib
    lib = _lib.load()
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    lib.cmlpl_debug_reload_switches()
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.cmlpl_debug_reload_switches()


def _scene(rows, cols, C_, bands, seed=99):
    rng = np.random.Generator(np.random.PCG64(seed))
    cube = rng.standard_normal((rows, cols, C_)).astype(np.float32)
    X = rng.standard_normal((rows * cols, bands)).astype(np.float32)
    return cube, X


def _params(shape, seed):
    p = O.closed_form_params(shape, seed)
    p["classifier.weight"] = p["classifier.weight"] * SCALE
    return p


def _module(shape, params):
    from cmlpl_amd.models import BaseNet2
    net = BaseNet2(num_features=shape.bands, dropout=0.8, num_classes=shape.K, in_channels=shape.C, window=shape.H).to(DEV)
    net.load_state_dict(params)
    net.eval()
    return net


def _forward(params, XP, X, dtype):
    with torch.no_grad():
        z, _ = O.basenet2_forward({k: v.to(dtype) for k, v in params.items()}, XP.to(dtype), X.to(dtype), None)
    return z.double()


@functools.lru_cache(maxsize=None)
def _host(cid):
    """a case's scene and the oracle on it, computed once: every pixel's window, the fp64 logits, the fp32 oracle's distance"""
    case = BY_ID[cid]
    s = O.NetShape(*case.shape)
    cube, X = _scene(case.rows, case.cols, s.C, s.bands)
    p = _params(s, 61)
    XP = torch.from_numpy(O.extract_patches(cube, s.H))
    want = _forward(p, XP, torch.from_numpy(X), torch.float64)
    own = float((_forward(p, XP, torch.from_numpy(X), torch.float32) - want).abs().max() / want.abs().max())
    return dict(case=case, s=s, cube=cube, X=X, p=p, XP=XP, want=want, own=own)


@functools.lru_cache(maxsize=None)
def _device(cid):
    """a case's scene on the device, its networks (seeds 61 and 62) and the whole-scene call of the first, computed once"""
    from cmlpl_amd.infer import infer_cube
    h = _host(cid)
    dc, dx = torch.from_numpy(h["cube"]).to(DEV), torch.from_numpy(h["X"]).to(DEV)
    nets = (_module(h["s"], h["p"]), _module(h["s"], _params(h["s"], 62)))
    labels, logits = infer_cube(nets[0], dc, dx, want_logits=True)
    torch.cuda.synchronize()
    return dict(cube=dc, X=dx, nets=nets, labels=labels, logits=logits)


def _hold(tag, why, labels, logits, want, own):
    """logits within BOUND of the largest fp64 logit; labels = _first_max of the device's logits everywhere, = the oracle's
    argmax away from its ties; -> the measured error"""
    from cmlpl_amd.infer import _first_max
    zmax = float(want.abs().max())
    got = logits.detach().cpu().double()
    assert got.shape == want.shape and labels.shape == (want.shape[0],) and labels.dtype == torch.int64
    err = float((got - want).abs().max() / zmax)
    bound = BOUND if own <= BOUND else 4 * own
    top2 = want.topk(2, dim=1).values if want.shape[1] > 1 else torch.cat([want, want - 1e30], 1)
    sure = (top2[:, 0] - top2[:, 1]) > 4 * BOUND * zmax
    left = 1.0 - float(sure.float().mean())
    print(f"[{tag}] {why}: logits {err:.2e} of max|z| = {zmax:.3g} (fp32 oracle {own:.2e}, bound {bound:.1e}); "
          f"{100 * left:.2f} % of {len(sure)} pixels within the tie margin")
    assert np.isfinite(err) and err < bound, (tag, err, own)
    assert torch.equal(labels, _first_max(logits)), "labels are not the first maximum of the device's own logits"
    assert left <= 0.02, left
    assert torch.equal(labels.cpu()[sure], want.argmax(1)[sure]), "labels differ from the oracle's away from ties"
    return err


def _route_on_device(s):
    from cmlpl_amd.infer import infer_fused
    return PATCHES if not infer_fused(s) else (FUSED4 if s.H * s.W <= 128 else FUSED8)


# ------------------------------------------------------------------ 1. against the oracle, in the case's route
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_logits_and_labels_against_the_fp64_oracle(case):
    from cmlpl_amd.infer import infer_supported
    h = _host(case.id)
    assert _route_on_device(h["s"]) == case.route and infer_supported(h["s"])
    d = _device(case.id)
    _hold(case.id, case.why, d["labels"], d["logits"], h["want"], h["own"])


# ------------------------------------------------------------------ 2. the feed, bit for bit
@pytest.mark.parametrize("case", FUSED, ids=[c.id for c in FUSED])
def test_ranges_chunks_and_lists_give_the_whole_scene_calls_bytes(case):
    from cmlpl_amd.infer import infer_cube, infer_pixels
    h, d = _host(case.id), _device(case.id)
    total = case.rows * case.cols
    net, dc, dx = d["nets"][0], d["cube"], d["X"]
    for n in (1, 7, 9):                     # a range that ends at the last pixel: a partly filled group of eight workgroups
        lab, z = infer_cube(net, dc, dx, pixel0=total - n, n=n, want_logits=True)
        assert _eq(z, d["logits"][total - n:]) and torch.equal(lab, d["labels"][total - n:]), n
    lab, z = infer_cube(net, dc, dx, chunk=8, want_logits=True)
    assert _eq(z, d["logits"]) and torch.equal(lab, d["labels"])
    # the list-fed call: both networks at once, a permutation with repeats, whole-scene rows and compact rows
    lab1, z1 = infer_cube(d["nets"][1], dc, dx, want_logits=True)
    assert not _eq(z1, d["logits"])
    whole = ((d["labels"], d["logits"]), (lab1, z1))
    rng = np.random.default_rng(3)
    pix_h = np.concatenate([rng.permutation(total), [total - 1, 0, 0, total // 2, total - 1]]).astype(np.int64)
    pix = torch.from_numpy(pix_h).to(DEV)
    for spectra, rows_ in ((dx, pix), (dx[pix].contiguous(), None)):
        lab2, z2 = infer_pixels(d["nets"], dc, spectra, pix, spec_rows=rows_, want_logits=True)
        assert z2.shape == (2, len(pix_h), h["s"].K) and lab2.shape == (2, len(pix_h))
        for k in range(2):
            assert _eq(z2[k], whole[k][1][pix]) and torch.equal(lab2[k], whole[k][0][pix]), (k, rows_ is None)


# ------------------------------------------------------------------ 3. views: the noise index on a second and third pass
@pytest.mark.parametrize("cid", VIEW_CASES)
def test_views_against_the_fp64_oracle_on_the_views_tensors(cid):
    """one noisy view, and one that is noisy under a spatial element that transposes (element 5), each through the
    range-fed and the list-fed forward, against the fp64 oracle on the tensors `views_of` returns (held to the view's
    definition by tests/test_gpu_tta.py part 1)"""
    from cmlpl_amd.tta import TTA, infer_cube_view, infer_pixels_view, views_of
    h, d = _host(cid), _device(cid)
    case, s = h["case"], h["s"]
    total = case.rows * case.cols
    dc, dx, net = d["cube"], d["X"], d["nets"][0]
    tta = TTA(3, 0.5, seed=1088)
    every = torch.arange(total, dtype=torch.int64, device=DEV)
    pix = torch.from_numpy(np.random.default_rng(5).permutation(total).astype(np.int64)).to(DEV)
    for t, g in ((2, 0), (1, 5)):
        XP, XS = views_of(dc, dx, every, s.H, tta, t, g=g)
        XP, XS = XP.cpu(), XS.cpu()
        assert float((XP - h["XP"]).abs().max()) > 0.5                  # (not the clean window)
        want = _forward(h["p"], XP, XS, torch.float64)
        own = float((_forward(h["p"], XP, XS, torch.float32) - want).abs().max() / want.abs().max())
        lab, z = infer_cube_view(net, dc, dx, tta, t, g=g)
        _hold(f"{cid} view {t} element {g}, range-fed", case.why, lab, z, want, own)
        lab_p, z_p = infer_pixels_view(net, dc, dx, pix, tta, t, spec_rows=pix, g=g)
        _hold(f"{cid} view {t} element {g}, list-fed", case.why, lab_p, z_p, want[pix.cpu()], own)
        assert _eq(z_p, z[pix]) and torch.equal(lab_p, lab[pix])        # a view belongs to the pixel, not to the feed


def test_views_of_the_largest_fused_case_without_the_view_cut():
    """256 channels at 14 x 14: no cut holds the window, so its views do not exist as tensors (`views_of` refuses).  What
    can be held without them: the PURE spatial element (sigma 0, the quarter turn) against the fp64 oracle on windows
    turned on the host by the element's definition -- the transposing gather on eight waves across three passes --, and the
    noisy view's independence of the feed, bit for bit.  The noise index itself on a third eight-wave pass is f8-c225's."""
    from cmlpl_amd import _lib
    from cmlpl_amd.tta import TTA, infer_cube_view, infer_pixels_view, views_of
    h, d = _host(VIEW_NO_CUT), _device(VIEW_NO_CUT)
    case, s = h["case"], h["s"]
    total = case.rows * case.cols
    dc, dx, net = d["cube"], d["X"], d["nets"][0]
    pix = torch.from_numpy(np.random.default_rng(5).permutation(total).astype(np.int64)).to(DEV)
    with pytest.raises(_lib.CmlplError) as e:
        views_of(dc, dx, pix, s.H, TTA(3, 0.5), 2)
    assert e.value.rc == -2
    XP = torch.from_numpy(apply_element(h["XP"].numpy(), 5))         # the definition, restated in tests/test_spatial_host.py
    assert torch.equal(XP[:, :, 0, 0], h["XP"][:, :, 0, s.H - 1]) and not torch.equal(XP, h["XP"])
    want = _forward(h["p"], XP, torch.from_numpy(h["X"]), torch.float64)
    own = float((_forward(h["p"], XP, torch.from_numpy(h["X"]), torch.float32) - want).abs().max() / want.abs().max())
    still = TTA(3, 0.0, seed=1088)
    lab, z = infer_cube_view(net, dc, dx, still, 1, g=5)
    _hold(f"{VIEW_NO_CUT} element 5 alone, range-fed", case.why, lab, z, want, own)
    lab_p, z_p = infer_pixels_view(net, dc, dx, pix, still, 1, spec_rows=pix, g=5)
    assert _eq(z_p, z[pix]) and torch.equal(lab_p, lab[pix])
    noisy = TTA(3, 0.5, seed=1088)
    lab_n, z_n = infer_cube_view(net, dc, dx, noisy, 1, g=5)
    lab_q, z_q = infer_pixels_view(net, dc, dx, pix, noisy, 1, spec_rows=pix, g=5)
    assert _eq(z_q, z_n[pix]) and torch.equal(lab_q, lab_n[pix])
    assert bool(torch.isfinite(z_n).all()) and float((z_n - z).abs().max()) > 1e-3 * float(want.abs().max())


# ------------------------------------------------------------------ 4. the fused cases, forced by patches
@pytest.mark.parametrize("cid", FORCED_BY_PATCHES)
def test_fused_cases_forced_by_patches_against_the_fp64_oracle(cid):
    from cmlpl_amd.infer import infer_cube, infer_fused, infer_supported
    h, d = _host(cid), _device(cid)
    with _switches({"CMLPL_FUSE_TAIL": "0"}):
        assert not infer_fused(h["s"]) and infer_supported(h["s"])
        labels, logits = infer_cube(d["nets"][0], d["cube"], d["X"], want_logits=True)
        torch.cuda.synchronize()
    assert infer_fused(h["s"])
    _hold(cid + " by patches", h["case"].why, labels, logits, h["want"], h["own"])


def _refused_before_a_launch(call, K, n):
    """`call(out)` must raise CmlplError rc -2 with nothing launched and nothing written"""
    from cmlpl_amd import _lib
    labels = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    logits = torch.full((n, K), -7.0, dtype=torch.float32, device=DEV)
    cnt = {}
    with _launch_counts(cnt):
        with pytest.raises(_lib.CmlplError) as e:
            call((labels, logits))
        torch.cuda.synchronize()
    assert e.value.rc == -2 and sum(cnt.values()) == 0, (e.value, cnt)
    assert bool((labels == -7).all()) and bool((logits == -7.0).all())


def test_the_largest_fused_case_is_refused_by_patches():
    """256 channels at 14 x 14: the fused kernel gathers it in chunks, no cut holds the window"""
    from cmlpl_amd.infer import infer_cube, infer_supported
    h, d = _host(FORCED_REFUSED), _device(FORCED_REFUSED)
    with _switches({"CMLPL_FUSE_TAIL": "0"}):
        assert not infer_supported(h["s"])
        _refused_before_a_launch(lambda out: infer_cube(d["nets"][0], d["cube"], d["X"], want_logits=True, out=out),
                                 h["s"].K, h["case"].rows * h["case"].cols)
    assert infer_supported(h["s"])


# ------------------------------------------------------------------ 5. the argmax rule
TIE = {"f4-c112": (3, 11, 4.0), "p-w7": (2, 7, 4.0)}          # (j, k, factor of rows j and k)


@pytest.mark.parametrize("cid", ARGMAX_CASES)
def test_the_first_maximum_wins_and_a_nan_is_the_maximum(cid):
    """torch.max's rule (reference tools/hyper_tools.py:430): ties between two identical classifier rows go to the first;
    a NaN logit is the maximum, the first NaN wins"""
    from cmlpl_amd.infer import infer_cube
    h, d = _host(cid), _device(cid)
    j, k, f = TIE[cid]
    n = h["case"].rows * h["case"].cols
    p = {key: v.clone() for key, v in h["p"].items()}
    p["classifier.weight"][j] *= f
    p["classifier.bias"][j] *= f
    p["classifier.weight"][k] = p["classifier.weight"][j]
    p["classifier.bias"][k] = p["classifier.bias"][j]
    want = _forward(p, h["XP"], torch.from_numpy(h["X"]), torch.float64)
    share = float((want.argmax(1) == j).float().mean())
    assert share >= 0.25 and bool((want[:, j] == want[:, k]).all()), share
    labels, logits = infer_cube(_module(h["s"], p), d["cube"], d["X"], want_logits=True)
    tied = (_bits(logits[:, j]) == _bits(logits[:, k])) & (logits[:, j] == logits.max(1).values)
    print(f"[{cid}] classes {j} = {k}: the oracle's argmax on {100 * share:.0f} % of {n} pixels, {int(tied.sum())} device ties at the maximum")
    assert int(tied.sum()) >= 10
    assert bool((labels[tied] == j).all()), "a tie did not go to the first maximum"
    for nans, winner in (((k,), k), ((j, k), j)):
        q = {key: v.clone() for key, v in h["p"].items()}
        for c in nans:
            q["classifier.bias"][c] = float("nan")
        lab, z = infer_cube(_module(h["s"], q), d["cube"], d["X"], want_logits=True)
        assert bool(torch.isnan(z[:, list(nans)]).all()) and int(torch.isnan(z).sum()) == n * len(nans)
        assert bool((lab == winner).all()), (nans, winner)


# ------------------------------------------------------------------ 6. refusals, before any launch
@pytest.mark.parametrize("cid,short", [("f4-c112", "rows"), ("f8-w13", "cols"), ("p-w7", "rows")])
def test_a_scene_smaller_than_half_a_window_is_refused_on_both_feeds(cid, short):
    from cmlpl_amd import _lib
    from cmlpl_amd.infer import infer_cube, infer_pixels
    from cmlpl_amd.tta import TTA, infer_cube_view, infer_pixels_view
    lib = _lib.load()
    h, d = _host(cid), _device(cid)
    s, net = h["s"], d["nets"][0]
    half = s.H // 2
    rows, cols = (half - 1, 16) if short == "rows" else (16, half - 1)
    n = rows * cols
    cube = torch.zeros(rows, cols, s.C, device=DEV)
    spectra = torch.zeros(n, s.bands, device=DEV)
    pix = torch.arange(n, dtype=torch.int64, device=DEV)
    tta = TTA(1, 0.5)
    for call in (lambda: infer_cube(net, cube, spectra), lambda: infer_pixels(net, cube, spectra, pix),
                 lambda: infer_cube_view(net, cube, spectra, tta, 0), lambda: infer_pixels_view(net, cube, spectra, pix, tta, 0)):
        with pytest.raises(ValueError, match=f"at least {half} x {half}"):
            call()
    if not h["case"].fused:
        return
    # the C calls: CMLPL_E_ARG, and the spectral launch in front of the gather has not run
    flat, packed = net._flat_params(net._live_params())
    labels = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    ws = torch.zeros(max(lib.cmlpl_infer_tta_workspace_bytes(C.byref(net._cshape), n), 1), dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    key = (C.c_float(0.5), C.c_uint64(1088), C.c_uint32(0), C.c_uint32(0))
    cnt = {}
    with _launch_counts(cnt):
        rcs = [lib.cmlpl_infer_cube(C.byref(net._cshape), flat.data_ptr(), packed.data_ptr(), cube.data_ptr(), rows, cols,
                                    spectra.data_ptr(), 0, n, labels.data_ptr(), None, ws.data_ptr(), ws.numel(), st),
               lib.cmlpl_infer_pixels(C.byref(net._cshape), 1, flat.data_ptr(), flat.numel(), packed.data_ptr(), packed.numel(),
                                      cube.data_ptr(), rows, cols, spectra.data_ptr(), None, pix.data_ptr(), n,
                                      labels.data_ptr(), None, ws.data_ptr(), ws.numel(), st),
               lib.cmlpl_infer_cube_tta_sym(C.byref(net._cshape), flat.data_ptr(), packed.data_ptr(), cube.data_ptr(), rows,
                                            cols, spectra.data_ptr(), 0, n, labels.data_ptr(), None, ws.data_ptr(),
                                            ws.numel(), st, *key),
               lib.cmlpl_infer_pixels_tta_sym(C.byref(net._cshape), 1, flat.data_ptr(), flat.numel(), packed.data_ptr(),
                                              packed.numel(), cube.data_ptr(), rows, cols, spectra.data_ptr(), None,
                                              pix.data_ptr(), n, labels.data_ptr(), None, ws.data_ptr(), ws.numel(), st, *key)]
        torch.cuda.synchronize()
    assert rcs == [-1, -1, -1, -1], rcs
    assert cnt["spe_fwd"] == 0 and sum(cnt.values()) == 0, cnt
    assert bool((labels == -7).all())


@pytest.mark.parametrize("shape", CUT_TOO_LARGE, ids=lambda s: "x".join(map(str, s)))
def test_a_window_no_cut_takes_is_refused_before_any_launch(shape):
    """103 raw bands under the reference's 20 x 20 window: `infer_supported` says no (so train.py's scene_source falls back),
    and a caller who goes ahead gets CMLPL_E_SHAPE from the constructor of the forward, not from its first chunk"""
    from cmlpl_amd.infer import infer_cube, infer_pixels, infer_supported
    from cmlpl_amd.tta import TTA, infer_cube_view
    s = O.NetShape(*shape)
    assert not infer_supported(s)
    rows, cols = s.H // 2 + 1, s.H // 2 + 2
    n = rows * cols
    net = _module(s, _params(s, 61))
    net._flat_params(net._live_params())            # (the weights are packed once, here: not a launch of the calls below)
    cube = torch.zeros(rows, cols, s.C, device=DEV)
    spectra = torch.zeros(n, s.bands, device=DEV)
    pix = torch.arange(n, dtype=torch.int64, device=DEV)
    _refused_before_a_launch(lambda out: infer_cube(net, cube, spectra, want_logits=True, out=out), s.K, n)
    _refused_before_a_launch(lambda out: infer_pixels(net, cube, spectra, pix, want_logits=True), s.K, n)
    _refused_before_a_launch(lambda out: infer_cube_view(net, cube, spectra, TTA(1, 0.5), 0), s.K, n)
