"""GPU: flip / rotate windows against their definition (include/cmlpl.h, "THE DEFINITION OF A SPATIAL ELEMENT"; restated
in numpy in tests/test_spatial_host.py: ``spatial_index``, ``training_elements``).

  1. cmlpl_tta_patches_sym: the remap is a pure permutation of ``extract_patches`` windows, the noise stays keyed by the
     output position -- bit for bit.
  2. The fused views (cmlpl_infer_cube_tta_sym / cmlpl_infer_pixels_tta_sym; by patches for 20 x 20) against the fp64 oracle
     forward on the ``views_of(..., g)`` windows, at the tolerance tests/test_gpu_tta.py:123-124 holds the noisy views to
     (1e-4 max |z| + 1e-5); sym = 0 through the new names gives the old names' bytes.
  3. The D4 orbit of an odd window makes the prediction invariant under a flip and a transposition of the scene.
  4. The cube-fed step with a spatial mode is the split-fed step on windows the HOST transformed per row, bit for bit.
  5. Its graph replay is the eager step, bit for bit.
  6. The two command lines.

The scene is 23 x 29 (rows and columns differ: a swapped axis shows); every pixel list holds the four corners, a pixel of
each margin and an interior one."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV, report
from tests.test_gpu_cube_feed import _explicit, _pixels, _same, _state
from tests.test_gpu_infer import _module, _scene
from tests.test_spatial_host import spatial_index, training_elements

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = 23, 29
SHAPES = {"B2": (103, 11, 11, 103, 9), "P": (60, 20, 20, 103, 9), "B5": (48, 15, 15, 48, 20)}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _eq(a, b):
    return torch.equal(_bits(a), _bits(b))


def _apply(win, g):
    """element g (an int, or one per window) of device windows [n, C, w, w], by ``spatial_index``"""
    n, Cc, w, _ = win.shape
    gs = [int(g)] * n if np.ndim(g) == 0 else [int(v) for v in g]
    idx = torch.from_numpy(np.stack([spatial_index(v, w) for v in gs])).to(win.device)
    return win.reshape(n, Cc, w * w).gather(2, idx[:, None, :].expand(n, Cc, w * w)).reshape(n, Cc, w, w).contiguous()


def _device_scene(shape, seed):
    cube_h, X_h = _scene(ROWS, COLS, shape[0], shape[3], seed)
    return torch.from_numpy(cube_h).to(DEV), torch.from_numpy(X_h).to(DEV)


def _list(w, n=13, seed=5):
    return _pixels(ROWS, COLS, w, n, torch.Generator().manual_seed(seed)).to(DEV)


# ------------------------------------------------------------------ 1. the views as tensors
@pytest.mark.parametrize("name", list(SHAPES))
def test_patches_are_permuted_windows_and_the_noise_stays_with_the_output_position(name):
    from cmlpl_amd.patches import extract_patches
    from cmlpl_amd.tta import TTA, views_of
    shape = SHAPES[name]
    w = shape[1]
    cube, _ = _device_scene(shape, 17)
    pix = _list(w)
    clean = extract_patches(cube, pix, w)
    zero = torch.zeros_like(cube)
    half0 = views_of(zero, None, pix, w, TTA(3, 0.5, seed=99), 1)[0]
    z = views_of(zero, None, pix, w, TTA(3, 1.0, seed=99), 1)[0]
    assert _eq(half0, z * 0.5) and float(z.abs().max()) > 1.0
    assert len({tuple(spatial_index(g, w)) for g in range(8)}) == 8
    for g in range(8):
        want = _apply(clean, g)
        got = views_of(cube, None, pix, w, TTA(3, 0.0, seed=99), 1, g=g)[0]
        assert _eq(got, want), f"{name} g {g}: sigma 0 is not the permuted window"
        if g:
            assert not _eq(want, clean)
        assert _eq(views_of(zero, None, pix, w, TTA(3, 0.5, seed=99), (1, g))[0], half0), f"{name} g {g}: the noise moved"
        # fmaf(z, 0.5, x): z / 2 is exact, so the fused product-sum is the rounded sum
        noisy = views_of(cube, None, pix, w, TTA(3, 0.5, seed=99), 1, g=g)[0]
        assert _eq(noisy, want + half0), f"{name} g {g}"
    # the clean block stays the clean window, and the spectra are not touched
    _, X = _device_scene(shape, 17)
    xp, x = views_of(cube, X, pix, w, TTA(3, 0.5, seed=99), 1, g=6)
    xp0, x0 = views_of(cube, X, pix, w, TTA(3, 0.5, seed=99), 1)
    assert _eq(x, x0) and _eq(xp, _apply(clean, 6) + half0) and not _eq(xp, xp0)
    assert _eq(views_of(cube, None, pix, w, TTA(3, 0.5, seed=99), None)[0], clean)


# ------------------------------------------------------------------ 2. the fused views
TOL = (1e-4, 1e-5)          # tests/test_gpu_tta.py:123-124: |got - want| <= 1e-4 max |want| + 1e-5 against the fp64 oracle
N_RANGE = 37                # the range: row 0 and eight pixels of row 1 -- two corners, the top margin, off the 8-pixel dealing


@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_views_match_the_oracle_on_the_transformed_windows(name):
    from cmlpl_amd.infer import infer_fused
    from cmlpl_amd.tta import TTA, infer_cube_view, infer_pixels_view, views_of
    shape = SHAPES[name]
    s = O.NetShape(*shape)
    assert infer_fused(s) == (name != "P")
    cube, X = _device_scene(shape, 99)
    net, p = _module(s, 61, scale=8.0)
    lst = _list(s.H)
    both = torch.cat([torch.arange(N_RANGE, dtype=torch.int64, device=DEV), lst])
    t = 2
    plain = infer_cube_view(net, cube, X, TTA(3, 0.0), t, n=N_RANGE)[1]
    for g in (1, 4, 6):
        for sigma in (0.0, 0.5):
            tta = TTA(3, sigma, seed=1088)
            XP, XS = views_of(cube, X, both, s.H, tta, t, g=g)
            with torch.no_grad():
                want, _ = O.basenet2_forward(p, XP.cpu(), XS.cpu(), None)
            atol = TOL[0] * float(want.abs().max()) + TOL[1]
            lab_r, z_r = infer_cube_view(net, cube, X, tta, (t, g), n=N_RANGE)
            lab_l, z_l = infer_pixels_view(net, cube, X, lst, tta, t, spec_rows=lst, g=g)
            report(f"[{name}] g {g} sigma {sigma}: range-fed logits vs the fp64 oracle", z_r, want[:N_RANGE], 0.0, atol)
            report(f"[{name}] g {g} sigma {sigma}: list-fed logits vs the fp64 oracle", z_l, want[N_RANGE:], 0.0, atol)
            top2 = want.topk(2, dim=1).values
            sure = ((top2[:, 0] - top2[:, 1]) > 2 * atol).to(DEV)
            assert torch.equal(torch.cat([lab_r, lab_l])[sure], want.argmax(1).to(DEV)[sure])
            assert float((z_r - plain).abs().max()) > 1e-3 * float(want.abs().max())      # not the window as it is
            # a chunked call, and two networks in one launch chain, see the same view
            assert _eq(infer_cube_view(net, cube, X, tta, t, n=N_RANGE, chunk=16, g=g)[1], z_r)
            z2 = infer_pixels_view((net, net), cube, X, lst, tta, (t, g), spec_rows=lst)[1]
            assert _eq(z2[0], z_l) and _eq(z2[1], z_l)


def _old_and_new_names(name, sigma):
    """every old entry point beside its _sym twin at sym = 0, called on the library itself: [(what, old bytes, new bytes)]"""
    from cmlpl_amd import _lib
    from cmlpl_amd.infer import _net_buffers, infer_fused
    shape = SHAPES[name]
    s = O.NetShape(*shape)
    lib = _lib.load()
    cube, X = _device_scene(shape, 3)
    lst = _list(s.H)
    n, K = lst.numel(), s.K
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    for sym in (None, 0):
        tail = () if sym is None else (sym,)
        sfx = "" if sym is None else "_sym"
        xp = torch.zeros(n, s.C, s.H, s.W, device=DEV)
        xs = torch.zeros(n, s.bands, device=DEV)
        _lib.check("patches", getattr(lib, "cmlpl_tta_patches" + sfx)(
            cube.data_ptr(), ROWS, COLS, s.C, s.H, lst.data_ptr(), n, xp.data_ptr(), X.data_ptr(), lst.data_ptr(), s.bands,
            xs.data_ptr(), sigma, 7, 1, st, *tail))
        res = [xp, xs]
        if infer_fused(s):
            net, _ = _module(s, 61, scale=8.0)
            cs, flat, packed = _net_buffers(net)
            ws = torch.empty(lib.cmlpl_eval_tta_workspace_bytes(C.byref(cs), 1, N_RANGE), dtype=torch.uint8, device=DEV)
            lab, z = torch.zeros(N_RANGE, dtype=torch.int64, device=DEV), torch.zeros(N_RANGE, K, device=DEV)
            _lib.check("cube", getattr(lib, "cmlpl_infer_cube_tta" + sfx)(
                C.byref(cs), flat.data_ptr(), packed.data_ptr(), cube.data_ptr(), ROWS, COLS, X.data_ptr(), 0, N_RANGE,
                lab.data_ptr(), z.data_ptr(), ws.data_ptr(), ws.numel(), st, sigma, 7, 1, *tail))
            lab2, z2 = torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(n, K, device=DEV)
            _lib.check("pixels", getattr(lib, "cmlpl_infer_pixels_tta" + sfx)(
                C.byref(cs), 1, flat.data_ptr(), flat.numel(), packed.data_ptr(), packed.numel(), cube.data_ptr(), ROWS, COLS,
                X.data_ptr(), lst.data_ptr(), lst.data_ptr(), n, lab2.data_ptr(), z2.data_ptr(), ws.data_ptr(), ws.numel(), st,
                sigma, 7, 1, *tail))
            res += [lab, z, lab2, z2]
        out.append(res)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("sigma", [0.0, 0.5])
@pytest.mark.parametrize("name", ["B2", "P"])
def test_the_identity_through_the_new_names_gives_the_old_names_bytes(name, sigma):
    old, new = _old_and_new_names(name, sigma)
    assert len(old) == (6 if name == "B2" else 2)
    for k, (a, b) in enumerate(zip(old, new)):
        assert _eq(a, b) and torch.isfinite(a.float()).all() and bool(a.any()), (name, sigma, k)


# ------------------------------------------------------------------ 3. invariance of the orbit's prediction
def _invariance(nets, cube, X, spatial):
    """max |p - p'| over corresponding pixels, and both label maps in the scene's own order, for the scene flipped
    left-right and the scene transposed"""
    from cmlpl_amd.tta import TTA, tta_cube
    tta = TTA(7, 0.0, clean=True, spatial=spatial)
    bands, Cc = X.shape[1], cube.shape[2]
    base = tta_cube(nets, cube, X, tta, probs=True)
    out = []
    for what, tf in (("flipped", lambda v: v.flip(1)), ("transposed", lambda v: v.transpose(0, 1))):
        cube_t = tf(cube).contiguous()
        X_t = tf(X.view(ROWS, COLS, bands)).contiguous()
        res = tta_cube(nets, cube_t, X_t.view(-1, bands), tta, probs=True)
        r2, c2 = cube_t.shape[:2]
        back = lambda v: tf(v.view(r2, c2, -1)).reshape(ROWS * COLS, -1)       # (both maps are their own inverses)
        out.append((what, back(res.probs), back(res.labels).view(-1)))
    return base, out


def test_the_d4_orbit_makes_the_prediction_invariant_under_flip_and_transposition():
    """Every view's window of the transformed scene is, bit for bit, another element's window of the scene (odd window:
    centred; the symmetric mirror commutes with the flip), so only the order of the 16 fp32 terms of sum <= 1 changes:
    15 x 2^-24 = 9e-7, doubled.  Labels where the top-2 margin exceeds 4e-6 (at most 1 % excluded: 0 pixels of 667 at this
    seed, by the fp64 oracle forward)."""
    shape = SHAPES["B2"]
    s = O.NetShape(*shape)
    cube, X = _device_scene(shape, 41)
    nets = [_module(s, 61, scale=8.0)[0], _module(s, 62, scale=8.0)[0]]
    base, moved = _invariance(nets, cube, X, "d4")
    top2 = base.probs.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 4e-6
    excluded = int((~sure).sum())
    for what, probs, labels in moved:
        d = float((probs - base.probs).abs().max())
        print("d4 orbit, scene %s: max |dp| %.3e (allowed 2e-6), %d of %d pixels inside the 4e-6 margin" %
              (what, d, excluded, sure.numel()))
        assert d <= 2e-6, what
        assert torch.equal(labels[sure], base.labels[sure]), what
    assert excluded <= 0.01 * sure.numel()
    # without the orbit the same comparison must NOT agree
    base0, moved0 = _invariance(nets, cube, X, "none")
    for what, probs, _ in moved0:
        d = float((probs - base0.probs).abs().max())
        print("no orbit, scene %s: max |dp| %.3e (must exceed 1e-4)" % (what, d))
        assert d > 1e-4, what


# ------------------------------------------------------------------ 4. training
def _train_scene(shape, n_lab, n_unl, seed):
    Cc, H, W, bands, K = shape
    g = torch.Generator().manual_seed(seed)
    cube = torch.randn(ROWS, COLS, Cc, generator=g)
    lab_pix, unl_pix = _pixels(ROWS, COLS, H, n_lab, g), _pixels(ROWS, COLS, H, n_unl, g)
    X = torch.randn(n_lab, bands, generator=g)
    Y = torch.randint(0, K, (n_lab,), generator=g)
    Xu = torch.randn(n_unl, bands, generator=g)
    return [t.to(DEV).contiguous() for t in (cube, lab_pix, unl_pix, X, Y, Xu)]


def _engine(shape, bt, btu, hist_rows=8, **kw):
    from cmlpl_amd import HyperParams, NetShape, TrainEngine
    eng = TrainEngine(NetShape(*shape), bt, btu, HyperParams(), device=DEV, seed=1088, hist_rows=hist_rows, **kw)
    eng.init_params_default(1088)
    return eng


TRAIN_CASES = [("B2", 24, 40, "d4", "cmlpl", False), ("B2", 24, 40, "d4", "cmlpl", True), ("P", 16, 16, "flips", "cmlpl", False),
               ("B5", 16, 48, "d4", "cps", False)]


@pytest.mark.parametrize("name,bt,btu,mode,method,explicit", TRAIN_CASES,
                         ids=["B2-d4", "B2-d4-noise8+dropmask", "P-flips", "B5-d4-cps"])
def test_the_cube_fed_step_with_a_mode_is_the_split_fed_step_on_host_transformed_windows(name, bt, btu, mode, method, explicit):
    from cmlpl_amd.patches import extract_patches
    shape = SHAPES[name]
    cube, lab_pix, unl_pix, X, Y, Xu = _train_scene(shape, bt, btu, 7)
    XP, XPu = extract_patches(cube, lab_pix, shape[1]), extract_patches(cube, unl_pix, shape[1])
    gen = torch.Generator().manual_seed(3)
    ea, eb = _engine(shape, bt, btu, method=method), _engine(shape, bt, btu, method=method, aug_spatial=mode)
    with pytest.raises(ValueError, match="cube-fed"):
        eb.step(XP, X, Y, XPu, Xu, 1, 0)
    assert ea.identity().get("aug_spatial") is None and eb.identity()["aug_spatial"] == mode
    for step in range(3):
        assert ea.step_count == eb.step_count == step
        # the rows' elements: global sample = batch row (labelled rows first), the step counter, the engine's seed
        g_rows = training_elements(1088, step, np.arange(bt + btu), mode)
        assert len(set(g_rows.tolist())) >= 4, (step, g_rows)
        assert g_rows.max() < (4 if mode == "flips" else 8)
        kw = {}
        if explicit:
            kw["noise"], kw["dropmask"] = _explicit(shape, bt, btu, gen)
        ea.step(_apply(XP, g_rows[:bt]), X, Y, _apply(XPu, g_rows[bt:]), Xu, 1, step, **kw)
        eb.step(None, X, Y, None, Xu, 1, step, cube=cube, lab_pix=lab_pix, unl_pix=unl_pix, **kw)
        xa, xb = ea.debug_region("xn"), eb.debug_region("xn")
        assert torch.equal(xa, xb), f"{name} step {step}: augmented rows differ, max |d| = {(xa - xb).abs().max().item():.3e}"
        (la, fa), (lb, fb) = ea.outputs(), eb.outputs()
        assert torch.equal(la, lb) and torch.equal(fa, fb), f"{name} step {step}: logits / features differ"
        _same(_state(ea), _state(eb), f"{name} step {step}")          # losses, gradients, parameters, moments, banks
    assert (ea.loss_window(3) == eb.loss_window(3)).all() and torch.isfinite(eb.scalar_hist[:3]).all()


def test_mode_none_is_the_engine_without_the_argument_and_a_mode_is_not():
    shape, bt, btu = SHAPES["B2"], 24, 40
    cube, lab_pix, unl_pix, X, Y, Xu = _train_scene(shape, bt, btu, 7)
    src = dict(cube=cube, lab_pix=lab_pix, unl_pix=unl_pix)
    ea, eb, ec = _engine(shape, bt, btu), _engine(shape, bt, btu, aug_spatial="none"), _engine(shape, bt, btu, aug_spatial="flips")
    for step in range(2):
        for e in (ea, eb, ec):
            e.step(None, X, Y, None, Xu, 1, step, **src)
    _same(_state(ea), _state(eb), "aug_spatial='none'")
    assert ea.identity() == eb.identity() and ea._io.reserved == eb._io.reserved == 0 and ec._io.reserved == 1 << 8
    assert not torch.equal(ea.params, ec.params)


# ------------------------------------------------------------------ 5. the captured step
def test_graph_replay_of_the_d4_step_is_bit_identical_to_eager():
    shape, bt, btu = SHAPES["B2"], 24, 40
    cube, lab_pix, unl_pix, X, Y, Xu = _train_scene(shape, 4 * bt + 5, 4 * btu + 3, 11)
    g = torch.Generator().manual_seed(5)
    lab_perm = torch.randperm(X.shape[0], generator=g).to(DEV)
    unl_perm = torch.randperm(Xu.shape[0], generator=g).to(DEV)
    sched = [(0, 15), (0, 16), (0, 17), (0, 18), (0, 19)]                     # one eager step, then 4 replays
    offs = [(k % 4) * bt for k in range(len(sched))], [(k % 4) * btu for k in range(len(sched))]
    src = dict(cube=cube, lab_pix=lab_pix, unl_pix=unl_pix)
    ea, eb, en = (_engine(shape, bt, btu, 16, aug_spatial=m) for m in ("d4", "d4", "none"))
    for k, (ep, bi) in enumerate(sched):
        for e in (ea, en):
            e.step(None, X, Y, None, Xu, ep, bi, lab_idx=lab_perm[offs[0][k]:offs[0][k] + bt],
                   unl_idx=unl_perm[offs[1][k]:offs[1][k] + btu], **src)
    ep, bi = sched[0]
    eb.step(None, X, Y, None, Xu, ep, bi, lab_idx=lab_perm[:bt], unl_idx=unl_perm[:btu], **src)
    graph = eb.capture(None, X, Y, None, Xu, lab_perm, unl_perm, bt, btu, capacity=16, **src)
    graph.program([(e, b, offs[0][k], offs[1][k]) for k, (e, b) in enumerate(sched)][1:])
    for _ in range(len(sched) - 1):
        graph.launch()
    torch.cuda.synchronize()
    assert ea.ptr == eb.ptr and ea.adam_t == eb.adam_t and ea.step_count == eb.step_count == len(sched)
    _same(_state(ea), _state(eb), "d4 after 5 steps")
    assert torch.isfinite(eb.scalar_hist[:len(sched)]).all()
    assert not torch.equal(ea.params, en.params)                               # (the replays did transform their windows)
    graph.close()


# ------------------------------------------------------------------ 6. the command lines
BASE = ["--synthetic", "B2", "--synthetic_scene", "--num_unlabel", "700", "--print_per_batches", "3", "--num_epochs", "2",
        "--no_eval", "--windows", "cube"]


def _py(script, *args, ok=True):
    r = subprocess.run([sys.executable, script, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r if not ok else r.stdout.splitlines()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("spatial"))
    f = lambda name: os.path.join(d, name)
    _py("train.py", *BASE, "--aug_spatial", "d4", "--ckpt_every", "1", "--save_ckpt", f("S{epoch}.pt"), "--save_loss_hist", f("S.npy"))
    return f


def test_a_resumed_leg_is_the_straight_run_and_another_mode_is_refused(runs):
    from cmlpl_amd import checkpoint
    f = runs
    _py("train.py", *BASE, "--aug_spatial", "d4", "--resume", f("S1.pt"), "--save_ckpt", f("R.pt"), "--save_loss_hist", f("R.npy"))
    assert np.load(f("R.npy")).tobytes() == np.load(f("S.npy")).tobytes()
    a, b = checkpoint.load(f("S2.pt")), checkpoint.load(f("R.pt"))
    for k in checkpoint.STATE_TENSORS:
        assert torch.equal(a[k], b[k]), k
    assert (a["ptr"], a["adam_t"], a["step_count"]) == (b["ptr"], b["adam_t"], b["step_count"])
    assert a["identity"]["aug_spatial"] == "d4" and a["extra"]["run"]["aug_spatial"] == "d4" and a["extra"]["args"]["aug_spatial"] == "d4"
    for other in (("--aug_spatial", "flips"), ()):
        r = _py("train.py", *BASE, *other, "--resume", f("S1.pt"), ok=False)
        assert r.returncode != 0 and "--aug_spatial d4" in r.stderr and "--aug_spatial %s" % (other[1] if other else "none") in r.stderr, \
            r.stderr[-2000:]
    # the augmentation did something: the same run without it has another loss history
    _py("train.py", *BASE, "--save_ckpt", f("N.pt"), "--save_loss_hist", f("N.npy"))
    assert np.load(f("N.npy")).tobytes() != np.load(f("S.npy")).tobytes()
    n = checkpoint.load(f("N.pt"))
    assert "aug_spatial" not in n["identity"] and "aug_spatial" not in n["extra"]["run"] and "aug_spatial" not in n["extra"]["args"]
    r = _py("train.py", *BASE[:-2], "--aug_spatial", "d4", ok=False)
    assert r.returncode != 0 and "--windows cube" in r.stderr


def test_predict_over_the_orbit(runs):
    f = runs
    n, K = 64 * 64, 9
    common = ("predict.py", "--ckpt", f("S2.pt"), "--synthetic", "B2", "--net", "ensemble", "--tta", "7", "--tta_noise", "0")
    got = _py(*common, "--tta_spatial", "d4", "--out", f("lab.npy"), "--proba", f("p.npy"))
    lab, p = np.load(f("lab.npy")), np.load(f("p.npy"))
    assert lab.shape == (n,) and lab.dtype == np.int64 and p.shape == (n, K) and p.dtype == np.float32
    assert np.array_equal(lab, p.argmax(1)) and np.abs(p.sum(1) - 1).max() < 1e-5
    assert [ln.split("=")[0] for ln in got if ln.startswith(" OA")] == [" OA_tta_d4"]
    assert sum(ln.startswith("producerA_tta_d4:") for ln in got) == 1 and sum(ln.startswith("AA_tta_d4=") for ln in got) == 1
    assert sum("tta inference time ==" in ln and "2 networks x 7 views + the clean window, noise 0, spatial d4)" in ln for ln in got) == 1
    # without --tta_spatial: the lines as they were
    plain = _py(*common, "--proba", f("p0.npy"))
    assert [ln.split("=")[0] for ln in plain if ln.startswith(" OA")] == [" OA_tta"]
    assert sum(ln.startswith("producerA_tta:") for ln in plain) == 1 and sum(ln.startswith("AA_tta=") for ln in plain) == 1
    assert sum(ln.endswith("(2 networks x 7 views + the clean window, noise 0)") for ln in plain) == 1
    assert not any("spatial" in ln or "_d4" in ln for ln in plain)
    assert np.abs(np.load(f("p0.npy")) - p).max() > 1e-6                      # eight clean windows are not the orbit
