"""CPU: the definition of a smoothed class probability map (include/cmlpl.h, "THE DEFINITION OF A SMOOTHED MAP") in fp64
numpy and the same arithmetic in fp32, the case builder of the GPU tests (tests/test_gpu_smooth.py), what the definition
promises on those cases, and the wiring of the feature that needs no device: ``Smooth``, the source list, the header,
the two command lines' refusals."""
import os
import re

import numpy as np
import pytest
import torch

from tests.test_ensemble_host import first_max, top2_margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-5


def constants(sigma_s, sigma_r):
    """a = fl32(1 / (2 sigma_s^2)), b = fl32(1 / (2 sigma_r^2)), formed in double from the fp32 arguments (inf: b = 0)"""
    ss, sr = float(np.float32(sigma_s)), float(np.float32(sigma_r))
    return np.float32(1.0 / (2.0 * ss * ss)), np.float32(0.0 if np.isinf(sr) else 1.0 / (2.0 * sr * sr))


def _fma32(x, y, z):
    """fmaf on float32 arrays: the product is exact in double, the sum rounds there once more before it rounds to fp32 --
    a double rounding that differs from fmaf in a handful of elements out of 2^29, far inside the yardstick's purpose"""
    return (np.asarray(x, np.float64) * np.asarray(y, np.float64) + np.asarray(z, np.float64)).astype(np.float32)


def smooth_def(p, guide, rows, cols, R, sigma_s, sigma_r, dt=np.float64):
    """The definition on p [rows * cols, K] and guide [rows, cols, G] (G may be 0): q, label, conf, entropy.  ``dt`` float64 is
    the definition, float32 the same operations in the same order in fp32 (the yardstick of the device's tolerance)."""
    K, G = p.shape[1], guide.shape[2]
    a, b = (dt(v) for v in constants(sigma_s, sigma_r))
    fma = _fma32 if dt is np.float32 else (lambda x, y, z: x * y + z)
    P, Gd = p.reshape(rows, cols, K).astype(dt), guide.astype(dt)
    num, den = np.zeros((rows, cols, K), dt), np.zeros((rows, cols), dt)
    with np.errstate(invalid="ignore", under="ignore"):
        for dy in range(-R, R + 1):                     # taps dy ascending, dx ascending within dy; those outside are left out
            for dx in range(-R, R + 1):
                y0, y1, x0, x1 = max(0, -dy), min(rows, rows - dy), max(0, -dx), min(cols, cols - dx)
                if y1 <= y0 or x1 <= x0:
                    continue
                d2 = np.zeros((y1 - y0, x1 - x0), dt)
                for c in range(G):                      # guide channels ascending
                    d = Gd[y0:y1, x0:x1, c] - Gd[y0 + dy:y1 + dy, x0 + dx:x1 + dx, c]
                    d2 = fma(d, d, d2)
                w = np.exp(-fma(d2, b, dt(dy * dy + dx * dx) * a)).astype(dt)
                num[y0:y1, x0:x1] = fma(w[..., None], P[y0 + dy:y1 + dy, x0 + dx:x1 + dx], num[y0:y1, x0:x1])
                den[y0:y1, x0:x1] = den[y0:y1, x0:x1] + w
        q = (num / den[..., None]).reshape(-1, K)
        q[np.isnan(q).any(1)] = np.nan                  # a NaN in any class is a NaN row
        label = first_max(q)
        s = np.zeros(len(q), dt)
        for c in range(K):                              # the entropy's sum runs c ascending
            qc = q[:, c]
            s = s + np.where(qc == 0, dt(0), qc * np.log(np.where(qc == 0, dt(1), qc)))
    return dict(q=q, label=label, conf=q[np.arange(len(q)), label], entropy=dt(0) - s)


def case(rows, cols, K, G, seed, channels=None, blk=7, sig=1.2, noise=0.5):
    """Regions of width ``blk`` with a seeded class each; guide = the class's prototype + ``noise`` N(0,1) in the first G of
    ``channels`` cube channels (the rest N(0,1): never read); p = softmax of ``sig`` N(0,1) with +1.5 on the true class.
    Returns p [rows * cols, K] f32, the cube [rows, cols, channels] f32 and the true classes."""
    rng = np.random.default_rng(seed)
    channels = G if channels is None else channels
    reg = rng.integers(0, K, ((rows + blk - 1) // blk, (cols + blk - 1) // blk))
    Y = np.repeat(np.repeat(reg, blk, 0), blk, 1)[:rows, :cols]
    proto = rng.standard_normal((K, G)) * 2
    cube = rng.standard_normal((rows, cols, channels)).astype(np.float32)
    cube[:, :, :G] = (proto[Y] + noise * rng.standard_normal((rows, cols, G))).astype(np.float32)
    z = (sig * rng.standard_normal((rows * cols, K))).astype(np.float32)
    z[np.arange(rows * cols), Y.reshape(-1)] += 1.5
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32), cube, Y.reshape(-1)


# (rows, cols, K, G, R): several regions each, K >= 2 so that there is something to get wrong
DEF_CASES = [(37, 29, 9, 3, 2), (19, 70, 16, 1, 4), (33, 33, 17, 4, 1), (40, 23, 64, 3, 3)]


@pytest.mark.parametrize("rows,cols,K,G,R", DEF_CASES)
def test_the_definition_on_the_builders_cases(rows, cols, K, G, R):
    p, cube, Y = case(rows, cols, K, G, 1)
    ref = smooth_def(p, cube[:, :, :G], rows, cols, R, 2.0, 1.0)
    raw, oa = (p.argmax(1) == Y).mean(), (ref["label"] == Y).mean()
    under = (top2_margin(ref["q"]) < MARGIN).mean()
    f32 = smooth_def(p, cube[:, :, :G], rows, cols, R, 2.0, 1.0, np.float32)
    print("%d x %d K %d G %d R %d: OA raw %.3f smoothed %.3f, under the margin %.4f, fp32 against fp64 %.2e"
          % (rows, cols, K, G, R, raw, oa, under, np.abs(f32["q"] - ref["q"]).max()))
    assert oa > raw
    assert np.abs(ref["q"].sum(1) - 1).max() <= 1e-6
    assert under <= 0.01
    assert f32["q"].dtype == np.float32 and np.abs(f32["q"] - ref["q"]).max() < 1e-6
    assert np.array_equal(ref["conf"], ref["q"].max(1)) and (ref["entropy"] >= 0).all()


def test_exact_properties_of_the_definition():
    p, cube, _ = case(9, 11, 5, 3, 2)
    for dt in (np.float64, np.float32):
        no_guide = smooth_def(p, cube[:, :, :0], 9, 11, 2, 1.0, 0.5, dt)
        inf = smooth_def(p, cube[:, :, :3], 9, 11, 2, 1.0, float("inf"), dt)
        assert no_guide["q"].tobytes() == inf["q"].tobytes() and np.array_equal(no_guide["label"], inf["label"])
        assert not np.array_equal(no_guide["q"], smooth_def(p, cube[:, :, :3], 9, 11, 2, 1.0, 0.5, dt)["q"])
    # a radius larger than the scene: every pixel sees the whole scene
    p, cube, _ = case(5, 3, 2, 3, 3)
    big = smooth_def(p, cube, 5, 3, 8, 4.0, float("inf"))
    assert np.isfinite(big["q"]).all() and np.abs(big["q"].sum(1) - 1).max() <= 1e-6
    flat = smooth_def(p, cube, 5, 3, 8, 1e6, float("inf"))["q"]          # (all weights 1: the scene's mean everywhere)
    assert np.abs(flat - p.astype(np.float64).mean(0)).max() < 1e-9
    one = smooth_def(p[:1], cube[:1, :1], 1, 1, 4, 2.0, 0.5)
    assert np.array_equal(one["q"], p[:1].astype(np.float64))           # one pixel: its centre tap alone, weight exactly 1
    # a NaN row spoils exactly the square of radius R around it, whole rows
    p, cube, _ = case(12, 13, 4, 2, 4)
    p[5 * 13 + 6, 2] = np.nan
    q = smooth_def(p, cube, 12, 13, 2, 1.0, 0.5)["q"].reshape(12, 13, 4)
    hit = np.zeros((12, 13), bool)
    hit[3:8, 4:9] = True
    assert np.isnan(q[hit]).all() and np.isfinite(q[~hit]).all()
    assert tuple(constants(2.0, float("inf"))) == (np.float32(0.125), np.float32(0.0))


# ------------------------------------------------------------------ wiring
def test_smooth_validation():
    from cmlpl_amd.smooth import Smooth, smooth_probs
    assert Smooth(4).params() == (4, 2.0, 0.5, 3, 1) and Smooth(3).params(60)[1] == 1.5
    assert Smooth(2, sigma_s=3.0, sigma_r=float("inf"), guide=8, iters=3).params(5) == (2, 3.0, float("inf"), 5, 3)
    assert Smooth(1, guide=0).params(60)[3] == 0
    for bad in (Smooth(0), Smooth(9), Smooth(2, sigma_s=0.0), Smooth(2, sigma_s=float("inf")), Smooth(2, sigma_s=float("nan")),
                Smooth(2, sigma_r=0.0), Smooth(2, sigma_r=-1.0), Smooth(2, sigma_r=float("nan")), Smooth(2, sigma_s=1e-30),
                Smooth(2, guide=-1), Smooth(2, guide=9), Smooth(2, iters=0)):
        with pytest.raises(ValueError, match="Smooth"):
            bad.params()
    assert "not tuned" in Smooth.__doc__.lower()
    with pytest.raises(ValueError, match="cuda"):
        smooth_probs(torch.zeros(12, 3), torch.zeros(3, 4, 5), Smooth(1))
    import cmlpl_amd
    assert cmlpl_amd.Smooth is Smooth and cmlpl_amd.smooth_probs is smooth_probs


def test_the_source_is_built_and_the_header_declares_the_export():
    from cmlpl_amd import _lib, build_ext
    assert "smooth.hip" in build_ext.SOURCES and "cmlpl_smooth_probs" in _lib.EXPORTS
    assert os.path.exists(os.path.join(ROOT, "cmlpl_amd", "csrc", "smooth.hip"))
    header = open(os.path.join(ROOT, "include", "cmlpl.h")).read()
    assert "#define CMLPL_ABI_VERSION 6" in header and "THE DEFINITION OF A SMOOTHED MAP" in header
    proto = re.search(r"\bint cmlpl_smooth_probs\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert proto is not None
    assert [a.split()[-1].lstrip("*") for a in proto.group(1).split(",")] == [
        "d_probs", "d_guide", "guide_stride", "guide_ch", "rows", "cols", "K", "radius", "sigma_s", "sigma_r", "d_out_probs",
        "d_labels", "d_conf", "d_entropy", "stream"]


def test_parsers_take_the_flags_and_refuse_what_they_cannot_mean():
    import predict
    import train
    from cmlpl_amd.smooth import Smooth
    q = predict.build_parser()
    a = q.parse_args(["--ckpt", "x"])
    assert (a.smooth, a.smooth_sigma_s, a.smooth_sigma_r, a.smooth_guide, a.smooth_iters) == (None,) * 5
    predict.check_args(a)
    for net in ("0", "1", "ema0", "ema1", "ensemble", "ensemble_all"):
        for more in ([], ["--tta", "2"]):
            predict.check_args(q.parse_args(["--ckpt", "x", "--net", net, "--smooth", "2", "--smooth_sigma_s", "1.5", "--smooth_sigma_r",
                                             "inf", "--smooth_guide", "0", "--smooth_iters", "2", "--proba", "p.npy", *more]))
    for net in ("both", "ema_both"):
        with pytest.raises(SystemExit) as e:
            predict.check_args(q.parse_args(["--ckpt", "x", "--net", net, "--smooth", "2"]))
        assert "--net " + net in str(e.value) and "--smooth" in str(e.value)
    bads = (["--smooth", "0"], ["--smooth", "9"], ["--smooth", "2", "--smooth_sigma_s", "0"], ["--smooth", "2", "--smooth_sigma_r", "-1"],
            ["--smooth", "2", "--smooth_guide", "9"], ["--smooth", "2", "--smooth_iters", "0"], ["--smooth_sigma_s", "1"],
            ["--smooth_sigma_r", "1"], ["--smooth_guide", "3"], ["--smooth_iters", "2"])
    for bad in bads:
        with pytest.raises(SystemExit):
            predict.check_args(q.parse_args(["--ckpt", "x", *bad]))
    p = train.build_parser()
    assert train.smooth_of(p.parse_args(["--synthetic", "B2"])) is None
    assert train.smooth_of(p.parse_args(["--synthetic", "B2", "--smooth", "2"])) == Smooth(2)
    assert train.smooth_of(p.parse_args(["--synthetic", "B2", "--smooth", "3", "--smooth_sigma_s", "2", "--smooth_sigma_r", "inf",
                                         "--smooth_guide", "1", "--smooth_iters", "2"])) == Smooth(3, 2.0, float("inf"), 1, 2)
    for bad in bads:
        with pytest.raises(SystemExit):
            train.smooth_of(p.parse_args(["--synthetic", "B2", *bad]))
    assert train.SMOOTH_TAG == "_smooth"


def test_refusals_come_before_any_device_call(monkeypatch):
    import predict
    import train

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch.cuda, "set_device", boom)
    with pytest.raises(SystemExit):
        predict.main(predict.build_parser().parse_args(["--ckpt", "nowhere.pt", "--net", "both", "--smooth", "2"]))
    with pytest.raises(SystemExit):
        predict.main(predict.build_parser().parse_args(["--ckpt", "nowhere.pt", "--smooth_guide", "2"]))
    for bad in (["--smooth_iters", "2"], ["--smooth", "12"]):
        with pytest.raises(SystemExit):
            train.main(train.build_parser().parse_args(["--synthetic", "B2", *bad]))


def test_saved_args_and_run_record_without_the_flag_are_what_they_were():
    import train
    from cmlpl_amd import HyperParams
    from tests.test_gpu_ema import PARENT_ARGS, PARENT_RUN
    p = train.build_parser()
    a0 = p.parse_args(["--synthetic", "B2"])
    a1 = p.parse_args(["--synthetic", "B2", "--smooth", "2", "--smooth_guide", "1"])
    s0, s1 = train.saved_args(a0), train.saved_args(a1)
    assert set(s0) == PARENT_ARGS
    assert s1["smooth"] == 2 and s1["smooth_guide"] == 1 and {k: v for k, v in s1.items() if not k.startswith("smooth")} == s0
    # smoothing is a way of LOOKING at a run: two legs of one run may differ in it
    r0, r1 = (train.run_record(a, HyperParams(), train.SYNTH["B2"], False) for a in (a0, a1))
    assert r0 == r1 and set(r0) == PARENT_RUN
