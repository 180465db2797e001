"""GPU: the three window gathers -- extract_patches_kernel (cmlpl_extract_patches), tta_patches_kernel (``views_of``) and
cube_feed_kernel (the rows a cube-fed training step leaves in its ``xn`` region) -- and augment_kernel (cmlpl_augment)
against the HOST reference of tests/window_cases.py over the whole table: the oracle's cut, ``spatial_index`` gathered
from it, the numpy generators.  tests/test_window_cases_cpu.py holds the table (which regime each case exists for).

Every comparison is BIT FOR BIT (the gather is a copy; fmaf(z, 0.5, x) is the rounded sum x + z / 2 because z / 2 is
exact) except where generated noise meets its numpy restatement: that is on a ZERO cube at sigma 1, within the project's
2e-5 for the hardware's log2 / sin / cos (tests/test_gpu_step.py, tests/test_gpu_tta.py).

No out-of-range pixel is ever fed to cmlpl_extract_patches or to a cube-fed step: unlike the TTA list (clamped on the
device, checked below) those lists are trusted by the kernels and range-checked on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import window_cases as W
from tests.test_spatial_host import spatial_index, training_elements
from tests.test_tta_host import view_window_noise
from tests.window_cases import BY_ID, EXTRACT, FEED, NOISE_TOL, TTA, cases_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x7FC0BEEF              # a NaN payload: no value of a seeded normal cube, of a sum with noise, or of the generator
SEED = 1088
E_ARG, E_SHAPE = -1, -2


def _ids(cases):
    return [c.id for c in cases]


def _i32(t):
    return t.contiguous().view(torch.int32)


def _same(got, want):
    """bit for bit, tensors on the device"""
    return got.shape == want.shape and torch.equal(_i32(got), _i32(want))


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)


def _sentinel(n):
    return torch.full((n,), SENT, dtype=torch.int32, device=DEV)


def _untouched(t):
    return bool((t.view(torch.int32) == SENT).all())


def _lib():
    from cmlpl_amd import _lib
    return _lib, _lib.load()


# ------------------------------------------------------------------ a. cmlpl_extract_patches
def _extract(cube, rows, cols, Cc, w, pix, n=None):
    """the raw call into a buffer one patch longer than the result, sentinel-filled: (rc, the n patches, the patch behind)"""
    _l, lib = _lib()
    n = pix.numel() if n is None else n
    per = Cc * w * w
    buf = _sentinel((max(n, 0) + 1) * per)
    rc = lib.cmlpl_extract_patches(cube.data_ptr(), rows, cols, Cc, w, pix.data_ptr(), n, buf.data_ptr(), _l.stream(cube.device))
    torch.cuda.synchronize()
    return rc, buf[:max(n, 0) * per], buf[max(n, 0) * per:]


@pytest.mark.parametrize("case", cases_for(EXTRACT), ids=_ids(cases_for(EXTRACT)))
def test_extract_patches_is_the_oracle_cut_and_writes_nothing_else(case):
    cube, pix = _dev(W.cube_of(case)), _dev(W.pixel_list(case))
    rc, got, behind = _extract(cube, case.rows, case.cols, case.C, case.w, pix)
    assert rc == 0
    want = W.cut_of(case)
    got_h = got.cpu().numpy()
    assert not (got_h == SENT).any(), "an element inside the result was never written"
    assert np.array_equal(got_h, want.reshape(-1).view(np.int32)), case.why
    assert _untouched(behind), "something was written behind the last patch"


def test_extract_patches_deals_every_list_length_exactly_once():
    case = BY_ID[W.DEALING_CASE]
    cube = _dev(W.cube_of(case))
    full = W.cut_of(case).reshape(len(W.pixel_list(case)), -1).view(np.int32)
    for n in W.DEALING_LENGTHS:
        pix = _dev(W.pixel_list(case)[:n])
        rc, got, behind = _extract(cube, case.rows, case.cols, case.C, case.w, pix)
        assert rc == 0 and _untouched(behind), n
        assert np.array_equal(got.cpu().numpy().reshape(n, -1), full[:n]), n
    # repeated and unsorted: the permuted result
    rng = np.random.default_rng(5)
    order = np.concatenate([rng.permutation(len(full))[:21], [3, 3, 0, len(full) - 1, 3]])
    rc, got, behind = _extract(cube, case.rows, case.cols, case.C, case.w, _dev(W.pixel_list(case)[order]))
    assert rc == 0 and _untouched(behind)
    assert np.array_equal(got.cpu().numpy().reshape(len(order), -1), full[order])


def test_extract_patches_refusals_launch_nothing():
    case = BY_ID["c5-w6"]
    Cc, w = case.C, case.w
    cube = _dev(W.cube_of(case))
    pix = torch.zeros(4, dtype=torch.int64, device=DEV)
    # a scene thinner than half a window (one mirror fold does not reach), either way: the cube's floats as such a scene
    for rows, cols in ((w // 2 - 1, case.cols), (case.rows, w // 2 - 1)):
        rc, got, behind = _extract(cube, rows, cols, Cc, w, pix)
        assert rc == E_SHAPE and _untouched(got) and _untouched(behind), (rows, cols)
    big = torch.zeros(3 * 3 * 103, device=DEV)                              # (a 3 x 3 scene of 103 bands; never read)
    rc, got, behind = _extract(big, 3, 3, W.CUT_REFUSED[0], W.CUT_REFUSED[1], pix[:1])
    assert rc == E_SHAPE and _untouched(got) and _untouched(behind)
    rc, got, behind = _extract(cube, case.rows, case.cols, Cc, w, pix, n=0)
    assert rc == E_ARG and _untouched(behind)


# ------------------------------------------------------------------ b. views_of (cmlpl_tta_patches_sym)
@pytest.mark.parametrize("case", cases_for(TTA), ids=_ids(cases_for(TTA)))
def test_views_are_the_oracle_cut_under_every_element_plus_the_documented_noise(case):
    from cmlpl_amd.tta import TTA as Tta, views_of
    Cc, w, ww = case.C, case.w, case.w * case.w
    pix_h = W.pixel_list(case)
    n = len(pix_h)
    cube, pix = _dev(W.cube_of(case)), _dev(pix_h)
    want = _dev(W.cut_of(case)).view(n, Cc, ww)
    under = lambda g: want[:, :, _dev(spatial_index(g, w))].view(n, Cc, w, w)
    for g in range(8):                                                      # sigma 0: pure geometry
        got, _ = views_of(cube, None, pix, w, Tta(1, 0.0, seed=SEED), 0, g=g)
        assert _same(got, under(g)), (case.id, g)
    # the noise alone: a zero cube at sigma 1, against the numpy generator
    t = 3
    zero = torch.zeros_like(cube)
    noise, _ = views_of(zero, None, pix, w, Tta(4, 1.0, seed=SEED), t)
    ref = np.stack([view_window_noise(SEED, t, int(P), Cc, w) for P in pix_h])
    err = float(np.abs(noise.cpu().numpy() - ref).max())
    print("%s: views, worst noise error %.2e (allowed %.0e)" % (case.id, err, NOISE_TOL))
    assert err <= NOISE_TOL
    # keyed by the output position: the same under an element; and added with one fma on the element's window
    for g in (0, 5):
        again, _ = views_of(zero, None, pix, w, Tta(4, 1.0, seed=SEED), t, g=g)
        assert _same(again, noise), g
        noisy, _ = views_of(cube, None, pix, w, Tta(4, 0.5, seed=SEED), t, g=g)
        assert _same(noisy, under(g) + 0.5 * noise), g
    # the documented clamp of the list: entries out of range show pixel 0 and the last pixel, noise and all
    last = case.rows * case.cols - 1
    odd = torch.tensor([-5, last + 4], dtype=torch.int64, device=DEV)
    ends = torch.tensor([0, last], dtype=torch.int64, device=DEV)
    for tta in (Tta(4, 0.0, seed=SEED), Tta(4, 0.5, seed=SEED)):
        a, _ = views_of(cube, None, odd, w, tta, t)
        b, _ = views_of(cube, None, ends, w, tta, t)
        assert _same(a, b)
    clean, _ = views_of(cube, None, odd, w, Tta(4, 0.0, seed=SEED), t)
    assert _same(clean, _dev(W.cut(case, [0, last])))


# ------------------------------------------------------------------ c. the cube-fed step's rows
BANDS, K = 5, 3


class Feed:
    """one cube-fed batch of a case: the scene, the pixel lists, spectra and labels (seeded), and the oracle's windows of
    the batch rows"""

    def __init__(self, case, bands=BANDS, spare=1):
        from tests.test_gpu_cube_feed import _pixels
        self.case, self.bands = case, bands
        self.shape = (case.C, case.w, case.w, bands, K)
        g = torch.Generator().manual_seed(31 + case.C)
        P = case.rows * case.cols
        if case.scene == "exact":                   # every pixel of the smallest scene, once
            self.bt, self.btu = (P + 1) // 2, P // 2
            every = torch.arange(P, dtype=torch.int64)
            lab, unl = every[:self.bt].repeat(spare), every[self.bt:].repeat(spare)
        else:                                       # corners, one pixel of each margin, the interior, a repeated pixel
            self.bt = self.btu = 12
            lab, unl = (_pixels(case.rows, case.cols, case.w, 12 * spare, g) for _ in range(2))
            lab[10], unl[11] = lab[4], unl[0]
        self.lab_h, self.unl_h = lab.numpy().copy(), unl.numpy().copy()
        self.cube = _dev(W.cube_of(case))
        self.lab_pix, self.unl_pix = lab.to(DEV), unl.to(DEV)
        self.X = torch.randn(len(lab), bands, generator=g).to(DEV)
        self.Y = torch.randint(0, K, (len(lab),), generator=g).to(DEV)
        self.Xu = torch.randn(len(unl), bands, generator=g).to(DEV)
        self.n = self.bt + self.btu
        self.per = W.per(case.C, case.w)

    def engine(self, sigma, mode="none"):
        from cmlpl_amd import HyperParams, NetShape, TrainEngine
        eng = TrainEngine(NetShape(*self.shape), self.bt, self.btu, HyperParams(noise=sigma), device=DEV, seed=SEED,
                          aug_spatial=mode)
        eng.init_params_default(SEED)
        return eng

    def rows(self, sigma, cube=None, mode="none", **kw):
        """the xn region [2][n][per] after the FIRST step (step counter 0) of a fresh engine at ``sigma``"""
        eng = self.engine(sigma, mode)
        eng.step(None, self.X, self.Y, None, self.Xu, 0, 0, cube=self.cube if cube is None else cube, lab_pix=self.lab_pix,
                 unl_pix=self.unl_pix, apply_update=False, **kw)
        torch.cuda.synchronize()
        assert eng.step_count == 1
        return eng.debug_region("xn").view(2, self.n, self.per).clone()

    def windows(self, lab_idx=None, unl_idx=None):
        """the oracle's windows of the batch rows [n, C, w, w] (numpy)"""
        lab = self.lab_h[:self.bt] if lab_idx is None else self.lab_h[lab_idx]
        unl = self.unl_h[:self.btu] if unl_idx is None else self.unl_h[unl_idx]
        return W.cut(self.case, np.concatenate([lab, unl]))

    def noise_reference(self, step=0):
        """[2][n][per]: the numpy generator under the documented counters (global sample = batch row, labelled first)"""
        return np.stack([np.stack([W.training_patch_noise(SEED, step, net, s, self.case.C, self.case.w)
                                   for s in W.global_samples(self.bt, self.btu)]) for net in range(2)])


def _check_three_modes(f, what, mode="none", lab_idx=None, unl_idx=None):
    """sigma 0, explicit draws at 0.5, in-kernel noise (zero cube at 1, the scene at 0.5) of one batch against the host
    reference; returns the device's noise rows"""
    from tests.test_gpu_cube_feed import _explicit
    kw = {} if lab_idx is None else dict(lab_idx=_dev(lab_idx), unl_idx=_dev(unl_idx))
    win = f.windows(lab_idx, unl_idx)
    if mode != "none":
        g_rows = training_elements(SEED, 0, W.global_samples(f.bt, f.btu), mode)
        assert g_rows.max() < (4 if mode == "flips" else 8) and len(set(g_rows.tolist())) >= 3, g_rows
        win = W.apply_elements(win, g_rows)
    clean_h = win.reshape(f.n, f.per)
    clean = _dev(clean_h)
    # 1. sigma == 0: both networks' rows are the cut
    got = f.rows(0.0, mode=mode, **kw)
    assert _same(got[0], clean) and _same(got[1], clean), (what, "sigma 0")
    # 2. explicit draws at 0.5: each network against ITS draws, in numpy float32
    gen = torch.Generator().manual_seed(3)
    noise, dm = _explicit(f.shape, f.bt, f.btu, gen)
    got = f.rows(0.5, mode=mode, noise=noise, dropmask=dm, **kw).cpu().numpy()
    for net in range(2):
        draw = np.concatenate([noise[2 * net].cpu().numpy().reshape(f.bt, f.per),
                               noise[4 + 2 * net].cpu().numpy().reshape(f.btu, f.per)])
        want = clean_h + np.float32(0.5) * draw
        assert want.dtype == np.float32
        assert np.array_equal(got[net].view(np.int32), want.view(np.int32)), (what, "explicit draws", net)
    assert not np.array_equal(got[0], got[1])
    # 3. in-kernel noise: the generator on a zero cube, then one fma on the scene
    z = f.rows(1.0, cube=torch.zeros_like(f.cube), mode=mode, **kw)
    err = float(np.abs(z.cpu().numpy() - f.noise_reference()).max())
    print("%s: cube feed, worst noise error %.2e (allowed %.0e)" % (what, err, NOISE_TOL))
    assert err <= NOISE_TOL, (what, err)
    got = f.rows(0.5, mode=mode, **kw)
    for net in range(2):
        assert _same(got[net], clean + 0.5 * z[net]), (what, "in-kernel noise", net)
    return z


FEED_CASES = cases_for(FEED)


@pytest.mark.parametrize("case", FEED_CASES, ids=_ids(FEED_CASES))
def test_cube_fed_rows_are_the_oracle_cut_plus_the_documented_noise(case):
    _check_three_modes(Feed(case), case.id)


def test_cube_fed_rows_with_the_unfused_spectral_launch():
    case = BY_ID[W.FEED_BANDS300]
    _check_three_modes(Feed(case, bands=300), case.id + "-bands300")


@pytest.mark.parametrize("name", W.FEED_BY_INDEX)
def test_cube_fed_rows_follow_the_index_and_the_noise_follows_the_batch_row(name):
    f = Feed(BY_ID[name], spare=3)                          # lists three times the batch
    rng = np.random.default_rng(11)
    lab_idx, unl_idx = rng.permutation(3 * f.bt)[:f.bt], rng.permutation(3 * f.btu)[:f.btu]
    assert (lab_idx >= f.bt).any() and (unl_idx >= f.btu).any()
    z = _check_three_modes(f, name + "-by-index", lab_idx=lab_idx.astype(np.int64), unl_idx=unl_idx.astype(np.int64))
    # the noise is the batch row's, whatever row of the lists it shows
    first = dict(lab_idx=_dev(np.arange(f.bt, dtype=np.int64)), unl_idx=_dev(np.arange(f.btu, dtype=np.int64)))
    assert _same(z, f.rows(1.0, cube=torch.zeros_like(f.cube), **first))


@pytest.mark.parametrize("mode", ["flips", "d4"])
@pytest.mark.parametrize("name", W.FEED_SPATIAL)
def test_cube_fed_rows_under_a_spatial_mode(name, mode):
    f = Feed(BY_ID[name])
    z = _check_three_modes(f, "%s-%s" % (name, mode), mode=mode)
    # keyed by the output position: the mode does not move the noise
    assert _same(z, f.rows(1.0, cube=torch.zeros_like(f.cube)))


@pytest.mark.parametrize("name", W.FEED_VS_SPLIT)
def test_the_split_fed_step_on_the_oracles_windows_leaves_the_same_rows(name):
    f = Feed(BY_ID[name])
    win = _dev(f.windows())
    ea, eb = f.engine(0.5), f.engine(0.5)
    ea.step(win[:f.bt].contiguous(), f.X, f.Y, win[f.bt:].contiguous(), f.Xu, 0, 0, apply_update=False)
    eb.step(None, f.X, f.Y, None, f.Xu, 0, 0, cube=f.cube, lab_pix=f.lab_pix, unl_pix=f.unl_pix, apply_update=False)
    torch.cuda.synchronize()
    xa, xb = ea.debug_region("xn"), eb.debug_region("xn")
    assert xa.numel() == 2 * f.n * f.per and _same(xa, xb)
    assert not _same(xb.view(2, f.n, f.per)[0], win.view(f.n, f.per))          # (noise was added)


@pytest.mark.parametrize("Cc,w", W.FEED_REFUSED)
def test_the_feed_refuses_a_window_past_its_lds_before_any_launch(Cc, w):
    from cmlpl_amd import HyperParams, NetShape, TrainEngine, _lib
    assert W.tile_lds(Cc, w) > W.LDS_MAX
    rows, cols, bt = w + 3, w + 2, 12
    eng = TrainEngine(NetShape(Cc, w, w, BANDS, K), bt, bt, HyperParams(), device=DEV, seed=SEED)
    eng.init_params_default(SEED)
    g = torch.Generator().manual_seed(1)
    cube = torch.randn(rows, cols, Cc, generator=g).to(DEV)
    pix = torch.randint(0, rows * cols, (bt,), generator=g).to(DEV)
    X, Y = torch.randn(bt, BANDS, generator=g).to(DEV), torch.randint(0, K, (bt,), generator=g).to(DEV)
    eng.workspace.fill_(0xA5)
    torch.cuda.synchronize()
    with pytest.raises((_lib.CmlplError, ValueError)) as e:
        eng.step(None, X, Y, None, X, 0, 0, cube=cube, lab_pix=pix, unl_pix=pix, apply_update=False)
    if isinstance(e.value, _lib.CmlplError):
        assert e.value.rc == E_SHAPE
    torch.cuda.synchronize()
    assert eng.step_count == 0 and eng.adam_t == 0
    assert bool((eng.workspace == 0xA5).all()), "a launch of the refused step wrote the workspace"


# ------------------------------------------------------------------ d. cmlpl_augment
AUG = [(W.AUGMENT_CASES[i % len(W.AUGMENT_CASES)], b) for i, b in enumerate(W.AUGMENT_BANDS)]


@pytest.mark.parametrize("nets", [1, 2])
@pytest.mark.parametrize("name,bands", AUG, ids=["%s-bands%d" % a for a in AUG])
def test_augment_is_a_copy_plus_the_documented_noise(name, bands, nets):
    _l, lib = _lib()
    case = BY_ID[name]
    Cc, w, per = case.C, case.w, W.per(case.C, case.w)
    cs = _l.Shape(Cc, w, w, bands, K)
    bt, btu, step = 3, 2, 3
    n = bt + btu
    g = torch.Generator().manual_seed(per + bands)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    xpl, xl, xpu, xu = rnd(bt, per), rnd(bt, bands), rnd(btu, per), rnd(btu, bands)
    st = _l.stream(torch.device(DEV))

    def run(src, sigma, noise8=None):
        xn, sn = _sentinel(2 * n * per), _sentinel(2 * n * bands)
        keep = None if noise8 is None else (C.c_void_p * 8)(*[t.data_ptr() for t in noise8])
        rc = lib.cmlpl_augment(C.byref(cs), nets, bt, btu, src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(),
                               src[3].data_ptr(), None if keep is None else C.cast(keep, C.POINTER(C.c_void_p)), sigma,
                               SEED, step, None, xn.data_ptr(), sn.data_ptr(), None, st)
        torch.cuda.synchronize()
        assert rc == 0
        if nets == 1:           # nothing where network 1's rows would start
            assert _untouched(xn[n * per:]) and _untouched(sn[n * bands:])
        return xn.view(torch.float32).view(2, n, per)[:nets], sn.view(torch.float32).view(2, n, bands)[:nets]

    real = (xpl, xl, xpu, xu)
    xp_all, x_all = torch.cat([xpl, xpu]), torch.cat([xl, xu])
    xn, sn = run(real, 0.0)                                                   # a copy: cat(XPl, XPu), cat(Xl, Xu)
    for net in range(nets):
        assert _same(xn[net], xp_all) and _same(sn[net], x_all), net
    draws = [rnd(*s) for s in [(bt, per), (bt, bands)] * 2 + [(btu, per), (btu, bands)] * 2]
    xn, sn = run(real, 0.5, draws)                                            # explicit draws: numpy float32
    for net in range(nets):
        zp = np.concatenate([draws[2 * net].cpu().numpy(), draws[4 + 2 * net].cpu().numpy()])
        zs = np.concatenate([draws[2 * net + 1].cpu().numpy(), draws[4 + 2 * net + 1].cpu().numpy()])
        want_p = xp_all.cpu().numpy() + np.float32(0.5) * zp
        want_s = x_all.cpu().numpy() + np.float32(0.5) * zs
        assert np.array_equal(xn[net].cpu().numpy().view(np.int32), want_p.view(np.int32)), net
        assert np.array_equal(sn[net].cpu().numpy().view(np.int32), want_s.view(np.int32)), net
    zeros = tuple(torch.zeros_like(t) for t in real)
    zn, zs = run(zeros, 1.0)                                                  # the generator itself
    for net in range(nets):
        ref_p = np.stack([W.training_patch_noise(SEED, step, net, s, Cc, w) for s in range(n)])
        ref_s = np.stack([W.training_spectrum_noise(SEED, step, net, s, bands) for s in range(n)])
        ep, es = float(np.abs(zn[net].cpu().numpy() - ref_p).max()), float(np.abs(zs[net].cpu().numpy() - ref_s).max())
        print("%s bands %d nets %d net %d: augment, worst noise error patches %.2e spectra %.2e (allowed %.0e)"
              % (name, bands, nets, net, ep, es, NOISE_TOL))
        assert ep <= NOISE_TOL and es <= NOISE_TOL
    xn, sn = run(real, 0.5)                                                   # and one fma on the rows
    for net in range(nets):
        assert _same(xn[net], xp_all + 0.5 * zn[net]) and _same(sn[net], x_all + 0.5 * zs[net]), net
