"""CPU: test-time augmentation without a device -- the definition of a VIEW (include/cmlpl.h) restated in numpy on the
generator of tests/test_noise_generator_math.py, the fp64 definition of the views ensemble that tests/test_gpu_tta.py holds
cmlpl_ensemble_views to, the exports and their argument checks (in front of any launch), and the command lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.test_ensemble_host import (case_logits, ensemble_fp64, first_max, normalised_weights, top2_margin)
from tests.test_noise_generator_math import _ctr, noise_normal4, noise_normal8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
FAKE = 0x10000
STREAM_TTA_XP, STREAM_TTA_X = 0x400, 0x500


# ------------------------------------------------------------------ section 1 of the definition, in numpy
def view_window_noise(seed, t, P, C, w):
    """z [C, w, w] of view t of scene pixel P: bands 8c .. 8c + 7 of window pixel p are hash call (P, pair p QP / 2 + c)"""
    ww, HQ = w * w, 2 * ((C + 15) // 16)                       # HQ = QP / 2 pairs of band quads per window pixel
    pairs = (np.arange(ww)[:, None] * HQ + np.arange(HQ)[None, :]).reshape(-1)
    z = noise_normal8(seed, t, STREAM_TTA_XP, _ctr(P, pairs))  # [8, ww * HQ]
    z = z.T.reshape(ww, HQ * 8)[:, :C]                         # [window pixel][band]
    return np.ascontiguousarray(z.T).reshape(C, w, w)


def view_window_noise_elementwise(seed, t, P, C, w, p, b):
    """the definition word for word, one element: component b & 3 of noise_normal4p(.., gsample = P, G = p QP + (b >> 2))"""
    QP = 4 * ((C + 15) // 16)
    G = p * QP + (b >> 2)
    z8 = noise_normal8(seed, t, STREAM_TTA_XP, _ctr(P, np.array([G >> 1])))[:, 0]     # noise_normal4p: pair G >> 1 ...
    return z8[4 * (G & 1) + (b & 3)]                                                   # ... its odd or even group


def view_spectrum_noise(seed, t, P, bands):
    q = np.arange((bands + 3) // 4)
    return noise_normal4(seed, t, STREAM_TTA_X, _ctr(P, q)).T.reshape(-1)[:bands]


def test_the_vectorised_restatement_is_the_definition():
    C, w = 103, 11
    z = view_window_noise(1088, 3, 77, C, w)
    for p, b in ((0, 0), (0, 7), (5, 8), (37, 50), (120, 102), (64, 99), (1, 3), (1, 4)):
        assert z[b, p // w, p % w] == view_window_noise_elementwise(1088, 3, 77, C, w, p, b), (p, b)


def test_moments_of_a_view():
    C, w = 103, 11
    z = np.concatenate([view_window_noise(1088, t, P, C, w).reshape(-1) for t in range(4) for P in range(24)])   # ~1.2 M
    n = z.size
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 4 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / n)
    assert abs((z ** 4).mean() - 3.0) < 5 * np.sqrt(96.0 / n)
    for thr, p in ((1.0, 0.31731), (2.0, 0.045500), (3.0, 0.0026998)):
        got = (np.abs(z) > thr).mean()
        assert abs(got - p) < 5 * np.sqrt(p * (1 - p) / n), (thr, got, p)
    assert np.abs(z).max() <= np.sqrt(32 * np.log(2.0)) + 1e-5
    s = np.concatenate([view_spectrum_noise(1088, t, P, 103) for t in range(8) for P in range(400)])
    assert abs(s.mean()) < 4 / np.sqrt(s.size) and abs(s.var() - 1.0) < 5 * np.sqrt(2.0 / s.size)
    # neighbours: along the bands of a window pixel (inside and across hash calls) and along the window
    one = view_window_noise(1088, 0, 5, C, w).reshape(C, -1)
    many = np.stack([view_window_noise(1088, 0, P, C, w).reshape(C, -1) for P in range(40)])          # [P][C][ww]
    for lag in (1, 2, 4, 8):
        c = np.corrcoef(many[:, :-lag].reshape(-1), many[:, lag:].reshape(-1))[0, 1]
        assert abs(c) < 5 / np.sqrt(many[:, lag:].size), ("bands", lag, c)
    c = np.corrcoef(many[:, :, :-1].reshape(-1), many[:, :, 1:].reshape(-1))[0, 1]
    assert abs(c) < 5 / np.sqrt(many[:, :, 1:].size), ("window", c)
    assert one.shape == (C, w * w)


def test_views_are_independent_across_t_P_seed_and_of_the_training_streams():
    C, w = 103, 11
    base = view_window_noise(1088, 0, 5, C, w).reshape(-1)
    n = base.size
    HQ = 2 * ((C + 15) // 16)
    pairs = (np.arange(w * w)[:, None] * HQ + np.arange(HQ)[None, :]).reshape(-1)
    raw = lambda stream: noise_normal8(1088, 0, stream, _ctr(5, pairs)).T.reshape(w * w, HQ * 8)[:, :C].T.reshape(-1)
    assert np.array_equal(raw(STREAM_TTA_XP), base)
    others = {"next view": view_window_noise(1088, 1, 5, C, w).reshape(-1),
              "next pixel": view_window_noise(1088, 0, 6, C, w).reshape(-1),
              "other seed": view_window_noise(1089, 0, 5, C, w).reshape(-1),
              "training patches, net 0 (0x100)": raw(0x100), "training patches, net 1 (0x101)": raw(0x101),
              "training spectra (0x200)": raw(0x200), "the views' spectra stream (0x500)": raw(STREAM_TTA_X)}
    for name, o in others.items():
        assert not np.array_equal(o, base), name
        assert abs(np.corrcoef(base, o)[0, 1]) < 5 / np.sqrt(n), name
    sb = np.concatenate([view_spectrum_noise(1088, 0, P, 103) for P in range(100)])
    for name, o in {"next view": np.concatenate([view_spectrum_noise(1088, 1, P, 103) for P in range(100)]),
                    "shifted pixels": np.concatenate([view_spectrum_noise(1088, 0, P + 1, 103) for P in range(100)]),
                    "training spectra (0x200)": np.concatenate(
                        [noise_normal4(1088, 0, 0x200, _ctr(P, np.arange(26))).T.reshape(-1)[:103] for P in range(100)])}.items():
        assert abs(np.corrcoef(sb, o)[0, 1]) < 5 / np.sqrt(sb.size), name
    # a view is a property of (seed, t, P) alone: formed again, anywhere, it is the same
    assert np.array_equal(view_window_noise(1088, 0, 5, C, w).reshape(-1), base)


def test_every_group_index_fits_the_counter():
    """noise_ctr keeps 24 bits for the group: G = p QP + (b >> 2) for windows up to 20 x 20 and C up to 256"""
    worst = 0
    for w in range(1, 21):
        for C in range(1, 257):
            QP = 4 * ((C + 15) // 16)
            worst = max(worst, (w * w - 1) * QP + ((C - 1) >> 2))
            assert ((C - 1) >> 2) < QP                         # a window pixel's groups do not run into the next pixel's
    assert worst < 2 ** 24 and worst == 399 * 64 + 63


# ------------------------------------------------------------------ the views ensemble, in numpy fp64
def views_weights(weights, M, V):
    """w_{m,v} = fl32(w_m / sum w / V), formed in double -- what the kernel receives, per member"""
    w = np.ones(M) if weights is None else np.asarray(weights, dtype=np.float64)
    return (w / w.sum() / V).astype(np.float32)


def ensemble_views_fp64(z, weights=None):
    """the definition on logits [M, V, n, K]: p = sum_m sum_v w_mv softmax(z_mv), m ascending, v ascending within m"""
    z = np.asarray(z, dtype=np.float64)
    M, V = z.shape[:2]
    w = views_weights(weights, M, V).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = np.exp(z - np.nanmax(np.where(np.isnan(z), -np.inf, z), axis=-1, keepdims=True))
        e = np.where(np.isnan(z).any(-1, keepdims=True), np.nan, e)
        pm = e / e.sum(-1, keepdims=True)
        p = np.zeros(z.shape[2:])
        for m in range(M):
            for v in range(V):
                p = p + w[m] * pm[m, v]
        label = first_max(p)
        t = np.where(p == 0, 0.0, p * np.log(np.where(p == 0, 1.0, p)))
        label_mv = first_max(pm)
    return dict(pm=pm, p=p, label=label, conf=np.take_along_axis(p, label[:, None], 1)[:, 0], entropy=-t.sum(-1),
                disagree=(label_mv != label[None, None]).sum((0, 1)).astype(np.int32), label_mv=label_mv)


def ensemble_views_fp32_torch(z, weights=None):
    """the same arithmetic in fp32 with torch on the CPU: its error against fp64 is the yardstick of the device's"""
    zt = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))
    M, V = zt.shape[:2]
    w = torch.from_numpy(views_weights(weights, M, V))
    pm = torch.softmax(zt, -1)
    p = torch.zeros_like(pm[0, 0])
    for m in range(M):
        for v in range(V):
            p = p + w[m] * pm[m, v]
    t = torch.where(p == 0, torch.zeros_like(p), p * torch.log(torch.where(p == 0, torch.ones_like(p), p)))
    return p.numpy(), (-t.sum(-1)).numpy()


# K, M, V: M V = 6, 12, 12, 64, 64, and K = 3 and 5 for the lane groups of 4 and 8 that the others leave out
VIEW_CASES = ((9, 2, 3), (9, 2, 6), (16, 4, 3), (20, 4, 16), (9, 1, 64), (3, 2, 3), (5, 2, 3))


def views_case(K, M, V, n=4099):
    return case_logits(K, M * V, n).reshape(M, V, n, K)


def test_views_definition_reduces_to_the_ensemble_at_one_view():
    for K, M, w in ((9, 2, None), (16, 4, (3, 1, 2, 2)), (2, 1, None), (20, 3, (1, 0, 5))):
        z = case_logits(K, M, n=513)
        a, b = ensemble_views_fp64(z[:, None], w), ensemble_fp64(z, w)
        for k in ("p", "label", "conf", "entropy", "disagree"):
            assert np.array_equal(a[k], b[k]), (K, M, k)
        assert np.array_equal(views_weights(w, M, 1), normalised_weights(w, M))


def test_views_definition_yardstick_and_margins_of_the_gpu_cases():
    """what tests/test_gpu_tta.py relies on: the fp32 restatement's own error is a few 1e-7 and not zero, and the label
    margin 1e-5 leaves out at most 1 % of every case"""
    for K, M, V in VIEW_CASES:
        z = views_case(K, M, V)
        ref = ensemble_views_fp64(z)
        p32, e32 = ensemble_views_fp32_torch(z)
        ep, ee = np.abs(p32 - ref["p"]).max(), np.abs(e32 - ref["entropy"]).max()
        out = float((top2_margin(ref["p"]) < 1e-5).mean())
        print("K %d M %d V %d: fp32 torch-CPU error p %.2e entropy %.2e, pixels under the margin %.4f" % (K, M, V, ep, ee, out))
        # worst case of an fp32 sum of M V terms that total 1 (each addition rounds a partial sum <= 1) on softmaxes a few
        # ulps off: (M V + 8) 2^-24; the entropy's K terms p log p move by at most |log p + 1| <= 16 times that each
        bound = (M * V + 8) * 2.0 ** -24
        assert 0 < ep < bound and 0 < ee < 16 * bound and out <= 0.01
        assert np.abs(ref["p"].sum(1) - 1).max() < 1e-6       # (the fp32 weights do not sum to 1 exactly)
        assert ref["disagree"].max() <= M * V


# ------------------------------------------------------------------ the exports
def _lib_loaded():
    from cmlpl_amd import _lib, build_ext
    if build_ext.needs_build():
        build_ext.build(verbose=False)
    return _lib, _lib.load()


NEW = ("cmlpl_infer_tta_workspace_bytes", "cmlpl_infer_cube_tta", "cmlpl_eval_tta_workspace_bytes", "cmlpl_infer_pixels_tta",
       "cmlpl_tta_patches", "cmlpl_ensemble_views")


def _prototype(code, name, ret="int"):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), code)
    assert m, name
    return [" ".join(p.split()[:-1]) + "*" * p.split()[-1].count("*") for p in m.group(1).split(",")]


def test_exports_header_binding_and_version():
    _lib, lib = _lib_loaded()
    for s in NEW:
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert _lib.ABI_VERSION == 6 and lib.cmlpl_abi_version() == 6           # added after ABI 6, no bump
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cmlpl.h")).read(), flags=re.S)
    tail = ["float", "uint64_t", "uint32_t"]
    assert _prototype(code, "cmlpl_infer_cube_tta") == _prototype(code, "cmlpl_infer_cube") + tail
    assert _prototype(code, "cmlpl_infer_pixels_tta") == _prototype(code, "cmlpl_infer_pixels") + tail
    assert _prototype(code, "cmlpl_infer_tta_workspace_bytes", "size_t") == _prototype(code, "cmlpl_infer_workspace_bytes", "size_t")
    assert _prototype(code, "cmlpl_eval_tta_workspace_bytes", "size_t") == _prototype(code, "cmlpl_eval_workspace_bytes", "size_t")
    assert _prototype(code, "cmlpl_ensemble_views") == ["const float*", "int", "int", "int64_t", "int64_t", "const float*", "int",
                                                        "int", "int64_t*", "float*", "float*", "float*", "int32_t*", "void*"]
    assert _prototype(code, "cmlpl_tta_patches")[:8] == _prototype(code, "cmlpl_extract_patches")[:8]
    assert re.search(r"CMLPL_STREAM_TTA_XP\s*=\s*0x400\b", code) and re.search(r"CMLPL_STREAM_TTA_X\s*=\s*0x500\b", code)
    assert list(lib.cmlpl_infer_cube_tta.argtypes[-3:]) == [C.c_float, C.c_uint64, C.c_uint32]
    assert list(lib.cmlpl_infer_cube_tta.argtypes[:-3]) == list(lib.cmlpl_infer_cube.argtypes)
    assert list(lib.cmlpl_infer_pixels_tta.argtypes[:-3]) == list(lib.cmlpl_infer_pixels.argtypes)
    assert lib.cmlpl_infer_tta_workspace_bytes.restype is C.c_size_t and lib.cmlpl_eval_tta_workspace_bytes.restype is C.c_size_t
    assert lib.cmlpl_ensemble_views.restype is C.c_int and lib.cmlpl_tta_patches.restype is C.c_int
    from cmlpl_amd import build_ext
    assert "tta.hip" in build_ext.SOURCES
    assert C.sizeof(_lib.StepIO) == 296 and C.sizeof(_lib.Dyn) == 64        # no record changed size
    import cmlpl_amd
    from cmlpl_amd import tta
    for name in ("TTA", "tta_cube", "tta_pixels", "views_of"):
        assert getattr(cmlpl_amd, name) is getattr(tta, name)
    # the workspace of a view: the clean call's, and the view's spectra rows behind it
    b2 = _lib.Shape(103, 11, 11, 103, 9)
    up = lambda v: (v + 255) & ~255
    assert lib.cmlpl_infer_tta_workspace_bytes(C.byref(b2), 100) == lib.cmlpl_infer_workspace_bytes(C.byref(b2), 100) + up(100 * 103 * 4)
    assert lib.cmlpl_eval_tta_workspace_bytes(C.byref(b2), 2, 100) == lib.cmlpl_eval_workspace_bytes(C.byref(b2), 2, 100) + up(100 * 103 * 4)
    p = _lib.Shape(60, 20, 20, 103, 9)                                      # by patches: not a shape the fused entries take
    assert lib.cmlpl_infer_tta_workspace_bytes(C.byref(p), 100) == 0 and lib.cmlpl_eval_tta_workspace_bytes(C.byref(p), 1, 100) == 0


def _views(lib, members=2, views=3, ms=None, vs=None, weights=None, n=16, K=9, logits=FAKE, labels=FAKE, probs=None):
    w = None if weights is None else (C.c_float * len(weights))(*weights)
    B = n * K
    return lib.cmlpl_ensemble_views(logits, members, views, views * B if ms is None else ms, B if vs is None else vs, w, n, K,
                                    labels, probs, None, None, None, None)


def test_ensemble_views_argument_checks_return_e_arg_before_any_launch():
    """every call here is refused on the host: had one launched, it would have failed another way on a machine without
    a device"""
    _, lib = _lib_loaded()
    B = 16 * 9
    for members, views in ((0, 1), (1, 0), (-1, 2), (2, -1), (65, 1), (1, 65), (5, 13), (8, 9), (64, 2), (2 ** 16, 2 ** 16)):
        assert _views(lib, members=members, views=views) == E_ARG, (members, views)
    for K in (0, 65, -3):
        assert _views(lib, K=K) == E_ARG, K
    for n in (0, -1):
        assert _views(lib, n=n) == E_ARG, n
    nan, inf = float("nan"), float("inf")
    for w in ((-1.0, 2.0), (nan, 1.0), (1.0, nan), (0.0, 0.0), (inf, 1.0), (1.0, -0.5)):
        assert _views(lib, weights=w) == E_ARG, w
    assert _views(lib, logits=None) == E_ARG and _views(lib, labels=None) == E_ARG
    assert _views(lib, logits=FAKE + 2) == E_ARG and _views(lib, labels=FAKE + 4) == E_ARG and _views(lib, probs=FAKE + 1) == E_ARG
    # blocks that overlap, either nesting
    assert _views(lib, vs=B - 1) == E_ARG and _views(lib, ms=3 * B - 1) == E_ARG
    assert _views(lib, ms=B - 1, vs=2 * B) == E_ARG and _views(lib, ms=B, vs=2 * B - 1) == E_ARG
    assert _views(lib, members=1, views=3, ms=0, vs=B - 1) == E_ARG
    assert _views(lib, members=3, views=1, ms=B - 1, vs=0) == E_ARG


def _fused(lib, which, sigma=0.5, n=16, pixel0=0, ws=FAKE, wsb=1 << 30, params=FAKE, pix=FAKE, nets=1, shape=(103, 11, 11, 103, 9)):
    from cmlpl_amd import _lib
    cs = _lib.Shape(*shape)
    if which == "cube":
        return lib.cmlpl_infer_cube_tta(C.byref(cs), params, FAKE, FAKE, 24, 20, FAKE, pixel0, n, FAKE, None, ws, wsb, None,
                                        sigma, 1088, 0)
    return lib.cmlpl_infer_pixels_tta(C.byref(cs), nets, params, 1 << 24, FAKE, 1 << 24, FAKE, 24, 20, FAKE, None, pix, n, FAKE,
                                      None, ws, wsb, None, sigma, 1088, 0)


def test_view_entry_points_refuse_bad_arguments_before_any_launch():
    _, lib = _lib_loaded()
    nan, inf = float("nan"), float("inf")
    for which in ("cube", "pixels"):
        for sigma in (-0.5, nan, inf, -inf):
            assert _fused(lib, which, sigma=sigma) == E_ARG, (which, sigma)
        assert _fused(lib, which, n=0) == E_ARG and _fused(lib, which, params=None) == E_ARG and _fused(lib, which, ws=None) == E_ARG
        assert _fused(lib, which, wsb=1024) == -3                           # CMLPL_E_WORKSPACE
        assert _fused(lib, which, shape=(60, 20, 20, 103, 9)) == -2         # CMLPL_E_SHAPE: this window goes by patches
    assert _fused(lib, "cube", pixel0=24 * 20 - 8) == E_ARG and _fused(lib, "cube", pixel0=-1) == E_ARG
    assert _fused(lib, "pixels", pix=None) == E_ARG and _fused(lib, "pixels", nets=3) == E_ARG
    f = lambda **k: lib.cmlpl_tta_patches(*[k.get(a, d) for a, d in (
        ("cube", FAKE), ("rows", 24), ("cols", 20), ("C", 103), ("w", 11), ("pix", FAKE), ("n", 8), ("out", FAKE), ("spectra", FAKE),
        ("spec_row", None), ("bands", 103), ("spectra_out", FAKE), ("sigma", 0.5), ("seed", 1088), ("view", 0), ("stream", None))])
    assert f(pix=None) == E_ARG and f(n=0) == E_ARG and f(sigma=-1.0) == E_ARG and f(sigma=nan) == E_ARG
    assert f(out=None, spectra_out=None) == E_ARG and f(cube=None) == E_ARG and f(spectra=None) == E_ARG and f(bands=0) == E_ARG
    assert f(w=50) == -2 and f(C=4000, w=20) == -2                          # half a window beyond the scene; the tile beyond LDS


def test_host_wrappers_refuse_what_they_cannot_take():
    from cmlpl_amd.tta import TTA, _check_blocks, ensemble_views_logits, views_of
    assert TTA(5, 0.5).blocks() == [None, 0, 1, 2, 3, 4] and TTA(2, 0.5, clean=False).blocks() == [0, 1]
    assert TTA(5, 0.5).seed == 1088 and TTA(5, 0.5).clean is True and TTA(0, 0.5).blocks() == [None]
    for bad in (TTA(-1, 0.5), TTA(0, 0.5, clean=False), TTA(3, -0.1), TTA(3, float("nan")), TTA(3, float("inf")), TTA(3, 0.5, seed=-1)):
        with pytest.raises(ValueError, match="TTA"):
            bad.blocks()
    assert len(_check_blocks(TTA(15, 0.5), 4)) == 16
    with pytest.raises(ValueError, match="64"):
        _check_blocks(TTA(16, 0.5), 4)
    with pytest.raises(ValueError, match="cuda"):
        ensemble_views_logits(torch.zeros(2, 3, 4, 9))
    with pytest.raises(ValueError, match="cuda"):
        views_of(torch.zeros(4, 4, 3), None, torch.zeros(2, dtype=torch.int64), 3, TTA(1, 0.5), 0)


# ------------------------------------------------------------------ the command lines
def test_parsers_take_the_new_flags():
    import predict
    import train
    p = train.build_parser()
    assert p.parse_args(["--synthetic", "B2"]).tta is False and p.parse_args(["--synthetic", "B2"]).m == 5
    a = p.parse_args(["--synthetic", "W8", "--tta", "--m", "2"])
    assert a.tta is True and a.m == 2 and train.SYNTH["W8"] == (40, 8, 8, 40, 5)
    assert train.NET_TAGS["tta"] == "_tta"
    q = predict.build_parser()
    a = q.parse_args(["--ckpt", "x"])
    assert a.tta is None and a.tta_noise is None and a.tta_seed == 1088 and a.tta_no_clean is False
    predict.check_args(a)
    for net in ("0", "1", "ema0", "ema1", "ensemble", "ensemble_all"):
        a = q.parse_args(["--ckpt", "x", "--net", net, "--tta", "3", "--tta_noise", "0.25", "--tta_seed", "7", "--tta_no_clean",
                          "--proba", "p.npy", "--confidence", "c.npy", "--entropy", "e.npy"])
        assert (a.tta, a.tta_noise, a.tta_seed, a.tta_no_clean) == (3, 0.25, 7, True)
        predict.check_args(a)
    for net in ("both", "ema_both"):
        with pytest.raises(SystemExit) as e:
            predict.check_args(q.parse_args(["--ckpt", "x", "--net", net, "--tta", "3"]))
        assert "--net " + net in str(e.value) and "--tta" in str(e.value)
    for bad in (["--tta", "0"], ["--tta", "64"], ["--tta", "3", "--tta_noise", "-1"], ["--tta", "3", "--tta_seed", "-1"],
                ["--tta_noise", "0.5"], ["--tta_no_clean"]):
        with pytest.raises(SystemExit):
            predict.check_args(q.parse_args(["--ckpt", "x", *bad]))


def test_tta_with_both_exits_before_any_device_call(monkeypatch):
    import predict

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch.cuda, "set_device", boom)
    with pytest.raises(SystemExit):
        predict.main(predict.build_parser().parse_args(["--ckpt", "nowhere.pt", "--net", "both", "--tta", "3"]))


def test_saved_args_and_run_record_without_the_flag_are_what_they_were():
    import train
    from cmlpl_amd import HyperParams
    from tests.test_gpu_ema import PARENT_ARGS, PARENT_RUN
    p = train.build_parser()
    a0 = p.parse_args(["--synthetic", "B2"])
    a1 = p.parse_args(["--synthetic", "B2", "--tta"])
    s0, s1 = train.saved_args(a0), train.saved_args(a1)
    assert "tta" not in s0 and set(s0) == PARENT_ARGS
    assert s1["tta"] is True and {k: v for k, v in s1.items() if k != "tta"} == s0
    # test-time augmentation is a way of LOOKING at a run: two legs of one run may differ in it
    r0, r1 = (train.run_record(a, HyperParams(), train.SYNTH["B2"], False) for a in (a0, a1))
    assert r0 == r1 and set(r0) == PARENT_RUN and train.run_differences(r0, r1) == []
