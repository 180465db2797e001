"""GPU: inference by pixel list (cmlpl_infer_pixels / cmlpl_amd.infer.infer_pixels) against ``infer_cube`` at the same
pixels -- labels AND logits, bit for bit, per network.  An equality and not a tolerance: each sample is one workgroup's
arithmetic on its own window, each spectral row depends on its own input row only, so neither the order of the list nor
the second network in the launch can change a bit.  ``infer_cube`` itself is held to the oracle by tests/test_gpu_infer.py
(whose scenes these are)."""
import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV
from tests.test_gpu_infer import _module, _scene

pytestmark = pytest.mark.gpu

SCENES = [("B2", (103, 11, 11, 103, 9), 64, 48), ("B4", (200, 11, 11, 200, 16), 20, 24),
          ("B5", (48, 15, 15, 48, 20), 24, 40), ("W8", (30, 8, 8, 30, 5), 16, 16),
          ("W12", (16, 12, 12, 16, 7), 14, 19), ("P", (60, 20, 20, 103, 9), 22, 26)]


def _lists(rows, cols, seed):
    n = rows * cols
    rng = np.random.Generator(np.random.PCG64(seed))
    corners = [0, cols - 1, (rows - 1) * cols, n - 1]
    edges = [cols // 2, (rows // 2) * cols, (rows // 2) * cols + cols - 1, (rows - 1) * cols + cols // 2]
    rep = np.concatenate([corners, edges, rng.integers(0, n, 301), corners, [n // 2] * 5])     # 322 items: repeats, not a multiple of 8
    return {"identity": np.arange(n), "permutation": rng.permutation(n), "repeats": rep}


@pytest.mark.parametrize("name,shape,rows,cols", SCENES)
def test_infer_pixels_equals_infer_cube_bit_for_bit(name, shape, rows, cols):
    from cmlpl_amd.infer import infer_cube, infer_pixels
    s = O.NetShape(*shape)
    cube, X = _scene(rows, cols, s.C, s.bands, 99)
    cube, X = torch.from_numpy(cube).to(DEV), torch.from_numpy(X).to(DEV)
    nets = [_module(s, 61, scale=8.0)[0], _module(s, 62, scale=5.0)[0]]
    want = [infer_cube(m, cube, X, want_logits=True) for m in nets]          # (labels [n], logits [n, K]) per network
    assert not torch.equal(want[0][1], want[1][1])
    for kind, lst in _lists(rows, cols, 5).items():
        pix = torch.from_numpy(lst.astype(np.int64)).to(DEV)
        # both networks in one call, spectra by pixel (infer_cube's addressing)
        lab2, log2 = infer_pixels(tuple(nets), cube, X, pix, spec_rows=pix, want_logits=True)
        assert lab2.shape == (2, len(lst)) and log2.shape == (2, len(lst), s.K)
        for k in range(2):
            assert torch.equal(lab2[k], want[k][0][pix]), (name, kind, k, "labels")
            assert torch.equal(log2[k], want[k][1][pix]), (name, kind, k, "logits")
            # ... equal one-network calls
            lab1, log1 = infer_pixels(nets[k], cube, X, pix, spec_rows=pix, want_logits=True)
            assert lab1.shape == (len(lst),)
            assert torch.equal(lab1, lab2[k]) and torch.equal(log1, log2[k]), (name, kind, k, "one network")
        # compact spectra (row i of the split = item i) equal spectra by pixel
        labc, logc = infer_pixels(tuple(nets), cube, X[pix].contiguous(), pix, want_logits=True)
        assert torch.equal(labc, lab2) and torch.equal(logc, log2), (name, kind, "compact")
    # labels alone (no logits buffer), and a list longer than a chunk (pieces of 100)
    pix = torch.from_numpy(_lists(rows, cols, 5)["permutation"].astype(np.int64)).to(DEV)
    lab = infer_pixels(tuple(nets), cube, X, pix, spec_rows=pix, chunk=100)
    assert torch.equal(lab[0], want[0][0][pix]) and torch.equal(lab[1], want[1][0][pix])


@pytest.mark.parametrize("n", [1, 13, 37])
def test_infer_pixels_short_lists(n):
    """n = 1, and n that is no multiple of 8 or 32 (the grid rounds up to 8 workgroups per XCD row, the spectral
    launch to 32 rows)"""
    from cmlpl_amd.infer import infer_cube, infer_pixels
    s = O.NetShape(103, 11, 11, 103, 9)
    rows, cols = 64, 48
    cube, X = _scene(rows, cols, s.C, s.bands, 99)
    cube, X = torch.from_numpy(cube).to(DEV), torch.from_numpy(X).to(DEV)
    nets = (_module(s, 61, scale=8.0)[0], _module(s, 62, scale=5.0)[0])
    rng = np.random.Generator(np.random.PCG64(n))
    pix = torch.from_numpy(rng.integers(0, rows * cols, n).astype(np.int64)).to(DEV)
    lab, log = infer_pixels(nets, cube, X, pix, spec_rows=pix, want_logits=True)
    for k in range(2):
        wl, wz = infer_cube(nets[k], cube, X, want_logits=True)
        assert torch.equal(lab[k], wl[pix]) and torch.equal(log[k], wz[pix])


def test_infer_pixels_refuses_lists_outside_the_scene():
    from cmlpl_amd.infer import infer_pixels
    s = O.NetShape(30, 8, 8, 30, 5)
    cube, X = _scene(16, 16, s.C, s.bands, 3)
    cube, X = torch.from_numpy(cube).to(DEV), torch.from_numpy(X).to(DEV)
    net = _module(s, 61)[0]
    for bad in ([0, 256], [-1, 3]):
        with pytest.raises(ValueError):
            infer_pixels(net, cube, X, torch.tensor(bad, dtype=torch.int64, device=DEV), spec_rows=torch.tensor([0, 1], device=DEV))
    with pytest.raises(ValueError):
        infer_pixels(net, cube, X, torch.tensor([0, 1], device=DEV), spec_rows=torch.tensor([0, 256], device=DEV))
