"""GPU: the smoothing kernel against its definition in fp64 (tests/test_smooth_host.py), its exact rules bit for bit, the
host functions against the calls they are made of, and the two command lines.

Tolerances -- the convention of tests/test_gpu_ensemble.py.  Probabilities, confidence and entropy: the yardstick is the
error of the SAME arithmetic in fp32 by numpy on the CPU against fp64 on the same inputs (0.4 .. 1.7e-7 for q on these
inputs); the device is allowed 8 x that per case, because its expf / logf are not libm's.  Labels: equal wherever the fp64
top-2 margin of q is >= 1e-5, which may leave out at most 1 % of a case (the definition alone leaves out at most 0.11 %)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV
from tests.test_ensemble_host import first_max, top2_margin
from tests.test_gpu_ensemble import B2, _engine, _py, _scene
from tests.test_smooth_host import MARGIN, case, smooth_def

pytestmark = pytest.mark.gpu
CHANNELS = 12                 # the cube of the kernel tests: guide_stride > G


def _run(p, cube, R, sigma_s, sigma_r, G, iters=1):
    """the kernel on p [rows * cols, K] under cube [rows, cols, C] (numpy): every output, as numpy"""
    from cmlpl_amd.smooth import Smooth, smooth_probs
    r = smooth_probs(torch.from_numpy(p).to(DEV), torch.from_numpy(np.ascontiguousarray(cube)).to(DEV),
                     Smooth(R, sigma_s, sigma_r, G, iters), probs_out=True, conf=True, entropy=True)
    torch.cuda.synchronize()
    assert r.labels.dtype == torch.int64 and r.probs.shape == p.shape and r.disagree is None
    return {k: getattr(r, k).cpu().numpy() for k in ("labels", "probs", "conf", "entropy")}


def _against_fp64(p, guide, rows, cols, R, sigma_s, sigma_r, got, tag):
    """``got`` (the device's q / conf / entropy / labels as numpy) against the definition on (p, guide)"""
    ref = smooth_def(p, guide, rows, cols, R, sigma_s, sigma_r)
    f32 = smooth_def(p, guide, rows, cols, R, sigma_s, sigma_r, np.float32)
    tol_q = 8 * np.abs(f32["q"] - ref["q"]).max()
    tol_e = 8 * np.abs(f32["entropy"] - ref["entropy"]).max()
    err_q = np.abs(got["probs"] - ref["q"]).max()
    err_c = np.abs(got["conf"] - ref["conf"]).max() if "conf" in got else 0.0
    err_e = np.abs(got["entropy"] - ref["entropy"]).max() if "entropy" in got else 0.0
    sure = top2_margin(ref["q"]) >= MARGIN
    print("%s %d x %d K %d G %d R %d: q err %.2e (allowed %.2e) conf err %.2e entropy err %.2e (allowed %.2e) under the margin %.4f"
          % (tag, rows, cols, p.shape[1], guide.shape[2], R, err_q, tol_q, err_c, err_e, tol_e, 1 - sure.mean()))
    assert err_q <= tol_q and err_c <= tol_q and err_e <= tol_e
    assert sure.mean() >= 0.99
    assert np.array_equal(got["labels"][sure], ref["label"][sure])
    assert ((got["labels"] >= 0) & (got["labels"] < p.shape[1])).all()
    return ref


# (rows, cols, K, G, R): every scene, K, G and R of the issue at least once, and the corner R = 8, K = 64, G = 8
KERNEL_CASES = [(37, 29, 9, 3, 2), (19, 70, 16, 1, 4), (5, 3, 2, 3, 4), (1, 1, 1, 0, 1), (37, 29, 17, 8, 1), (19, 70, 64, 8, 8),
                (37, 29, 1, 0, 8), (19, 70, 2, 0, 2), (5, 3, 64, 1, 8)]


@pytest.mark.parametrize("rows,cols,K,G,R", KERNEL_CASES)
def test_kernel_against_fp64(rows, cols, K, G, R):
    p, cube, _ = case(rows, cols, K, G, 1, channels=CHANNELS)
    got = _run(p, cube, R, 2.0, 1.0, G)
    _against_fp64(p, cube[:, :, :G], rows, cols, R, 2.0, 1.0, got, "kernel")
    assert np.array_equal(got["labels"], first_max(got["probs"])) and np.array_equal(got["conf"], got["probs"].max(1))
    if K == 1:
        assert (got["probs"] == 1).all() and (got["entropy"] == 0).all() and (got["labels"] == 0).all()
    if rows * cols == 1:
        assert got["probs"].tobytes() == p.tobytes()              # the centre tap alone, weight exactly 1


# ------------------------------------------------------------------ the exact rules, bit for bit
def test_two_runs_give_the_same_bytes():
    p, cube, _ = case(37, 29, 17, 3, 2, channels=CHANNELS)
    a, b = _run(p, cube, 4, 2.0, 1.0, 3), _run(p, cube, 4, 2.0, 1.0, 3)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("K,G,R", [(9, 3, 2), (17, 8, 4)])
def test_a_pixels_result_does_not_depend_on_the_tile(K, G, R):
    """a crop at an offset that is no multiple of the 32 x 8 tile: every pixel at least R from the crop's border sees
    the same neighbourhood as in the full scene, and must get the same bytes"""
    rows, cols, y0, x0, h, w = 40, 75, 5, 13, 30, 55
    p, cube, _ = case(rows, cols, K, G, 3, channels=CHANNELS)
    full = _run(p, cube, R, 2.0, 1.0, G)
    crop = _run(np.ascontiguousarray(p.reshape(rows, cols, K)[y0:y0 + h, x0:x0 + w]).reshape(h * w, K),
                cube[y0:y0 + h, x0:x0 + w], R, 2.0, 1.0, G)
    inner = (slice(R, h - R), slice(R, w - R))
    outer = (slice(y0 + R, y0 + h - R), slice(x0 + R, x0 + w - R))
    for k in full:
        a = crop[k].reshape(h, w, -1)[inner]
        b = full[k].reshape(rows, cols, -1)[outer]
        assert a.tobytes() == b.tobytes(), k
    assert crop["probs"].reshape(h, w, K)[0].tobytes() != full["probs"].reshape(rows, cols, K)[y0, x0:x0 + w].tobytes()


def test_no_guide_is_an_infinite_sigma_r():
    p, cube, _ = case(19, 70, 9, 3, 4, channels=CHANNELS)
    none, inf = _run(p, cube, 2, 1.0, 0.5, 0), _run(p, cube, 2, 1.0, float("inf"), 3)
    for k in none:
        assert none[k].tobytes() == inf[k].tobytes(), k
    assert not np.array_equal(none["probs"], _run(p, cube, 2, 1.0, 0.5, 3)["probs"])


def test_uniform_probabilities_stay_uniform():
    """a constant guide and a huge sigma_s: every weight is exactly 1, the sums of 1 / 16 are exact"""
    rows, cols, K = 19, 70, 16
    p = np.full((rows * cols, K), 1.0 / K, np.float32)
    cube = np.full((rows, cols, CHANNELS), 0.75, np.float32)
    got = _run(p, cube, 8, 1e15, 0.5, 8)
    assert got["probs"].tobytes() == p.tobytes() and (got["labels"] == 0).all() and (got["conf"] == np.float32(1.0 / K)).all()
    assert np.abs(got["entropy"] - np.log(K)).max() < 1e-6 and len(np.unique(got["entropy"])) == 1


@pytest.mark.parametrize("K,a,b", [(9, 6, 2), (17, 3, 16), (64, 50, 20), (2, 1, 0)])
def test_equal_tops_give_the_lower_index(K, a, b):
    rng = np.random.default_rng(5)
    rows, cols = 19, 70
    p = (0.2 * rng.dirichlet(np.ones(K), rows * cols)).astype(np.float32)
    top = (0.4 + 0.05 * rng.random(rows * cols)).astype(np.float32)
    p[:, a] = top
    p[:, b] = top                                     # the same map for both classes: the same arithmetic, the same bits
    _, cube, _ = case(rows, cols, K, 3, 6, channels=CHANNELS)
    got = _run(p, cube, 2, 1.0, 1.0, 3)
    assert got["probs"][:, a].tobytes() == got["probs"][:, b].tobytes()
    assert (got["labels"] == min(a, b)).all() and np.array_equal(got["conf"], got["probs"][:, a])


@pytest.mark.parametrize("K,c,R", [(9, 4, 2), (17, 16, 4), (9, 0, 8)])
def test_a_nan_row_spoils_exactly_the_pixels_within_the_radius(K, c, R):
    rows, cols, y, x = 37, 45, 15, 30
    p, cube, _ = case(rows, cols, K, 3, 7, channels=CHANNELS)
    clean = _run(p, cube, R, 0.7, 0.5, 3)             # (a narrow sigma_s: the far taps' weights underflow to 0 at R = 8)
    p[y * cols + x, c] = np.nan
    got = _run(p, cube, R, 0.7, 0.5, 3)
    hit = np.zeros((rows, cols), bool)
    hit[max(0, y - R):y + R + 1, max(0, x - R):x + R + 1] = True
    hit = hit.reshape(-1)
    assert np.isnan(got["probs"][hit]).all() and np.isnan(got["conf"][hit]).all() and np.isnan(got["entropy"][hit]).all()
    assert (got["labels"][hit] == 0).all()            # a NaN is the maximum, the first NaN wins
    for k in got:
        assert got[k][~hit].tobytes() == clean[k][~hit].tobytes(), k
    assert np.isfinite(got["probs"][~hit]).all()


def test_two_passes_are_two_calls():
    p, cube, _ = case(37, 29, 9, 3, 8, channels=CHANNELS)
    once = _run(p, cube, 2, 1.0, 0.5, 3)
    twice = _run(once["probs"], cube, 2, 1.0, 0.5, 3)
    for iters, want in ((2, twice), (3, _run(twice["probs"], cube, 2, 1.0, 0.5, 3))):
        got = _run(p, cube, 2, 1.0, 0.5, 3, iters=iters)
        for k in got:
            assert got[k].tobytes() == want[k].tobytes(), (iters, k)


def test_only_what_was_asked_for_is_returned():
    from cmlpl_amd.smooth import Smooth, smooth_probs
    p, cube, _ = case(19, 70, 9, 3, 9, channels=CHANNELS)
    pt, ct = torch.from_numpy(p).to(DEV), torch.from_numpy(cube).to(DEV)
    full = smooth_probs(pt, ct, Smooth(2), conf=True, entropy=True)
    bare = smooth_probs(pt, ct, Smooth(2), probs_out=False)
    assert bare.probs is None and bare.conf is None and bare.entropy is None and torch.equal(bare.labels, full.labels)
    assert torch.equal(pt.cpu(), torch.from_numpy(p))             # the input is left as it is
    two = ct[:, :, :2].contiguous()                               # the guide is clamped to the cube's channels
    assert torch.equal(smooth_probs(pt, two, Smooth(2, guide=8)).probs, smooth_probs(pt, two, Smooth(2, guide=2)).probs)
    with pytest.raises(ValueError, match="whole map"):
        smooth_probs(pt[:100], ct, Smooth(2))


# ------------------------------------------------------------------ the host functions
@pytest.fixture(scope="module")
def b2():
    eng = _engine(B2)
    cube, X = _scene(B2, 24, 20, 21)
    return eng, cube, X


def _same(a, b, what):
    for k in ("labels", "probs", "conf", "entropy"):
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), (what, k)


def test_smooth_cube_is_the_ensemble_then_the_filter(b2):
    from cmlpl_amd.ensemble import ensemble_cube
    from cmlpl_amd.smooth import Smooth, smooth_cube, smooth_probs
    from cmlpl_amd.tta import TTA, tta_cube
    eng, cube, X = b2
    sm = Smooth(2, sigma_r=2.0)
    ask = dict(probs=True, conf=True, entropy=True)
    raw = ensemble_cube((eng, None), cube, X, probs=True)
    want = smooth_probs(raw.probs, cube, sm, probs_out=True, conf=True, entropy=True)
    _same(smooth_cube((eng, None), cube, X, sm, **ask), want, "pair")
    _same(smooth_cube([(eng, 0), (eng, 1)], cube, X, sm, chunk=200, **ask), want, "two entries, in chunks")
    assert torch.isfinite(want.probs).all() and not torch.equal(want.probs, raw.probs)
    tta = TTA(2, 0.5, seed=7)
    raw_t = tta_cube((eng, None), cube, X, tta, probs=True)
    _same(smooth_cube((eng, None), cube, X, sm, tta=tta, **ask),
          smooth_probs(raw_t.probs, cube, sm, probs_out=True, conf=True, entropy=True), "tta")
    w = smooth_cube((eng, None), cube, X, sm, weights=(3, 1), probs=True)
    assert torch.equal(w.probs, smooth_probs(ensemble_cube((eng, None), cube, X, weights=(3, 1), probs=True).probs, cube, sm).probs)
    bare = smooth_cube((eng, 0), cube, X, sm)
    assert bare.probs is None and bare.labels.shape == (24 * 20,)


def test_the_library_refuses_what_it_cannot_take():
    from cmlpl_amd import _lib
    lib = _lib.load()
    rows, cols, K = 6, 7, 5
    p = torch.rand(rows * cols + 2, K, device=DEV)
    g = torch.rand(rows, cols, 4, device=DEV)
    out = torch.full((rows * cols + 2, K), 7.0, device=DEV)
    lab = torch.full((rows * cols + 1,), -7, dtype=torch.int64, device=DEV)
    ok = dict(p=p.data_ptr(), g=g.data_ptr(), gs=4, G=3, rows=rows, cols=cols, K=K, R=2, ss=1.0, sr=0.5, out=out.data_ptr(),
              lab=lab.data_ptr(), conf=None, ent=None)
    inf, nan = float("inf"), float("nan")
    bad = [dict(K=0), dict(K=65), dict(R=0), dict(R=9), dict(G=-1), dict(G=9), dict(rows=0), dict(cols=0), dict(g=None), dict(gs=2),
           dict(ss=0.0), dict(ss=-1.0), dict(ss=inf), dict(ss=nan), dict(sr=0.0), dict(sr=-0.5), dict(sr=nan), dict(ss=1e-30),
           dict(p=None), dict(out=None, lab=None), dict(p=p.data_ptr() + 2), dict(out=out.data_ptr() + 2), dict(g=g.data_ptr() + 1),
           dict(lab=lab.data_ptr() + 4), dict(conf=out.data_ptr() + 1), dict(ent=out.data_ptr() + 3),
           dict(out=p.data_ptr()), dict(out=p.data_ptr() + 4 * K), dict(out=p.data_ptr() + 4 * (rows * cols * K - 1)),
           dict(p=out.data_ptr() + 8 * K)]
    call = lambda a: lib.cmlpl_smooth_probs(a["p"], a["g"], a["gs"], a["G"], a["rows"], a["cols"], a["K"], a["R"], a["ss"], a["sr"],
                                            a["out"], a["lab"], a["conf"], a["ent"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for change in bad:
        assert call(dict(ok, **change)) == -1, change
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (lab == -7).all()               # nothing was launched
    for change in (dict(), dict(sr=inf), dict(G=0, g=None), dict(lab=None), dict(out=None), dict(gs=3)):
        assert call(dict(ok, **change)) == 0, change
    torch.cuda.synchronize()
    assert (out[rows * cols:] == 7.0).all() and lab[-1] == -7 and torch.isfinite(out).all()


# ------------------------------------------------------------------ the command lines
RUN = ["--synthetic", "B2", "--num_epochs", "1", "--synthetic_scene", "--num_unlabel", "128", "--labeled_batch_size", "32",
       "--unlabeled_batch_size", "32", "--print_per_batches", "2"]
RESULT = ("Result:", " OA", "producerA", "AA")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("smooth"))
    f = lambda name: os.path.join(d, name)
    out = _py("train.py", *RUN, "--smooth", "2", "--save_loss_hist", f("S.npy"), "--save_ckpt", f("S.pt"))
    plain = _py("train.py", *RUN, "--save_loss_hist", f("plain.npy"))
    return dict(out=out, plain=plain, f=f)


def test_train_with_smooth_adds_one_result_block_and_leaves_the_run_alone(runs):
    out, plain, f = runs["out"], runs["plain"], runs["f"]
    assert [ln.split("=")[0] for ln in out if ln.startswith(" OA")] == [" OA", " OA1", " OA_ens_smooth"]
    assert sum(ln.startswith("producerA_ens_smooth:") for ln in out) == 1 and sum(ln.startswith("AA_ens_smooth=") for ln in out) == 1
    assert sum("smoothing time ==" in ln and "radius 2" in ln for ln in out) == 1
    assert np.load(f("S.npy")).tobytes() == np.load(f("plain.npy")).tobytes()
    assert not any("smooth" in ln for ln in plain)
    i = next(k for k, ln in enumerate(out) if ln.startswith("ensemble inference time"))
    results = lambda lines: [ln for ln in lines if ln.startswith(RESULT) or ln.startswith("[")]
    assert results(out[:i]) == results(plain) and len(results(plain)) >= 8 and len(out) - i <= 12


@pytest.mark.parametrize("tta", [None, "2"], ids=["ensemble", "tta"])
def test_predict_with_smooth(runs, tta):
    import train
    from hsi_loader import SyntheticScene
    f = runs["f"]
    n, K = 64 * 64, B2[4]
    more = [] if tta is None else ["--tta", tta]
    tag = "_ens" if tta is None else "_tta"
    got = _py("predict.py", "--ckpt", f("S.pt"), "--synthetic", "B2", "--net", "ensemble", *more, "--smooth", "2", "--out", f("lab.npy"),
              "--proba", f("q.npy"), "--confidence", f("c.npy"), "--entropy", f("e.npy"))
    raw = _py("predict.py", "--ckpt", f("S.pt"), "--synthetic", "B2", "--net", "ensemble", *more, "--out", f("lab0.npy"),
              "--proba", f("p.npy"))
    assert [ln.split("=")[0] for ln in got if ln.startswith(" OA")] == [" OA" + tag, " OA" + tag + "_smooth"]
    assert [ln.split("=")[0] for ln in raw if ln.startswith(" OA")] == [" OA" + tag]
    results = lambda lines: [ln for ln in lines if ln.startswith(RESULT) or ln.startswith("[")]
    assert results(got)[:len(results(raw))] == results(raw)                 # the raw block is printed as it is without the flag
    lab, q, c, e, p = (np.load(f(x)) for x in ("lab.npy", "q.npy", "c.npy", "e.npy", "p.npy"))
    assert lab.shape == (n,) and lab.dtype == np.int64 and q.shape == (n, K) and q.dtype == np.float32
    assert np.array_equal(lab, first_max(q)) and np.array_equal(c, q.max(1)) and e.shape == (n,) and (e >= 0).all()
    guide = SyntheticScene(train.SYNTH["B2"], 64, 64, seed=3).cube_source(torch.device(DEV)).cube[:, :, :3].cpu().numpy()
    _against_fp64(p, guide, 64, 64, 2, 1.0, 0.5, dict(probs=q, conf=c, entropy=e, labels=lab), "predict.py " + tag)
    if tta is None:
        assert [ln for ln in got if ln.startswith(" OA_ens_smooth")] == [ln for ln in runs["out"] if ln.startswith(" OA_ens_smooth")]


def test_predict_one_network_with_smooth(runs):
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("S.pt"), "--synthetic", "B2", "--net", "1", "--smooth", "2", "--smooth_guide", "0",
              "--smooth_iters", "2", "--out", f("lab1.npy"), "--proba", f("q1.npy"))
    assert [ln.split("=")[0] for ln in got if ln.startswith(" OA")] == [" OA1", " OA1_smooth"]
    assert [ln for ln in got if ln.startswith(" OA1=")] == [ln for ln in runs["out"] if ln.startswith(" OA1=")]
    assert np.array_equal(np.load(f("lab1.npy")), first_max(np.load(f("q1.npy"))))
