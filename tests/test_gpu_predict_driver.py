"""GPU: the prediction functions are one chunk loop (cmlpl_amd.infer._predict) over one forward object -- what that makes
equal, held bit for bit at a fused shape (B2) and at one that goes by patches (P), every EnsembleResult field asked for:

  1. ``ensemble_*`` is ``tta_*`` with the one clean block;
  2. ``infer_*`` is the clean view of ``infer_*_view`` -- by patches too, where ``infer_pixels_view`` used to refuse;
  3. ``Evaluator.evaluate`` allocates nothing once its buffers exist."""
import numpy as np
import pytest
import torch

from tests.gpu_util import DEV
from tests.test_gpu_ensemble import ASK, B2, P, _engine, _same, _scene

pytestmark = pytest.mark.gpu
CASES = {"B2": (B2, 20, 24, 100, 64), "P": (P, 24, 20, 100, 64)}      # (64 pixels in chunks of 24: 24, 24 and a tail of 16)


def _eq(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    shape, rows, cols, pixel0, n = CASES[request.param]
    eng = _engine(shape)
    cube, X = _scene(shape, rows, cols, 41)
    run = torch.arange(pixel0, pixel0 + n, dtype=torch.int64, device=DEV)
    return dict(name=request.param, eng=eng, cube=cube, X=X, pixel0=pixel0, n=n, run=run, compact=X[run].contiguous())


def test_one_clean_block_is_the_ensemble(case):
    from cmlpl_amd.ensemble import ensemble_cube, ensemble_pixels
    from cmlpl_amd.tta import TTA, tta_cube, tta_pixels
    c = case
    eng, cube, X, run = c["eng"], c["cube"], c["X"], c["run"]
    clean = TTA(0, 0.0, clean=True)
    for nets in ((eng, None), [(eng, 0), (eng, 1)]):
        for chunk in (65536, 24):
            what = (c["name"], "pair" if isinstance(nets, tuple) else "two entries", chunk)
            _same(ensemble_cube(nets, cube, X, pixel0=c["pixel0"], n=c["n"], chunk=chunk, **ASK),
                  tta_cube(nets, cube, X, clean, pixel0=c["pixel0"], n=c["n"], chunk=chunk, **ASK), what + ("cube",))
            _same(ensemble_pixels(nets, cube, X, run, spec_rows=run, chunk=chunk, **ASK),
                  tta_pixels(nets, cube, X, run, clean, spec_rows=run, chunk=chunk, **ASK), what + ("pixels, spec_rows",))
            _same(ensemble_pixels(nets, cube, c["compact"], run, chunk=chunk, **ASK),
                  tta_pixels(nets, cube, c["compact"], run, clean, chunk=chunk, **ASK), what + ("pixels, compact rows",))


def test_plain_forward_is_the_clean_view(case):
    from cmlpl_amd.infer import infer_cube, infer_pixels
    from cmlpl_amd.tta import TTA, infer_cube_view, infer_pixels_view
    c = case
    eng, cube, X, run = c["eng"], c["cube"], c["X"], c["run"]
    tta = TTA(2, 0.5, seed=7)
    lab0, z0 = infer_cube((eng, 0), cube, X, pixel0=c["pixel0"], n=c["n"], want_logits=True)
    lab_v, z_v = infer_cube_view((eng, 0), cube, X, tta, None, pixel0=c["pixel0"], n=c["n"])
    assert _eq(z0, z_v) and torch.equal(lab0, lab_v) and torch.isfinite(z0).all()
    for nets in ((eng, 1), (eng, None)):
        lab, z = infer_pixels(nets, cube, X, run, spec_rows=run, want_logits=True)
        lab_v, z_v = infer_pixels_view(nets, cube, X, run, tta, None, spec_rows=run)
        assert z.shape == z_v.shape and _eq(z, z_v) and torch.equal(lab, lab_v), nets[1]
    if c["name"] == "P":            # by patches: the list-fed view is the range-fed one, clean and noisy
        for t in (None, 1):
            lab_c, z_c = infer_cube_view((eng, 0), cube, X, tta, t, pixel0=100, n=64)
            lab_p, z_p = infer_pixels_view((eng, 0), cube, X, run, tta, t, spec_rows=run)
            assert _eq(z_c, z_p) and torch.equal(lab_c, lab_p), t
        assert not _eq(z_c, z0)     # (view 1 is not the clean window)


def test_evaluate_does_not_allocate():
    from cmlpl_amd import NetShape
    from cmlpl_amd.evaluate import Evaluator
    from cmlpl_amd.infer import infer_pixels
    eng = _engine(B2)
    cube, X = _scene(B2, 20, 24, 43)
    K = B2[4]
    rng = np.random.default_rng(5)
    pix = torch.from_numpy(rng.permutation(20 * 24)[:200].astype(np.int64)).to(DEV)
    truth_h = rng.integers(0, K, 200).astype(np.int64)
    ev = Evaluator(NetShape(*B2), cube, X, torch.from_numpy(truth_h).to(DEV), pix, spec_rows=pix)
    first = {e: ev.evaluate((eng, None), ensemble=e).cpu().numpy().copy() for e in (False, True)}     # the warm calls
    for e in (False, True):
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        cm = ev.evaluate((eng, None), ensemble=e)
        torch.cuda.synchronize()
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before, e
        assert cm.cpu().numpy().tobytes() == first[e].tobytes()
    labels = infer_pixels((eng, None), cube, X, pix, spec_rows=pix).cpu().numpy()
    for k in range(2):
        want = np.zeros((K, K), np.int64)
        np.add.at(want, (truth_h, labels[k]), 1)
        assert np.array_equal(first[False][k], want) and np.array_equal(first[True][k], want), k
