"""GPU: the loss block of the cross-pseudo-supervision baseline alone (cmlpl_cps_loss_fwd_bwd, one launch) against
torch on given logits -- reference trian_CPS.py:234-258."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cmlpl_amd import _lib
from tests.gpu_util import DEV, report

pytestmark = pytest.mark.gpu
W = 0.1
HIST_RTOL = 1e-4          # the scalars' tolerance of tests/test_gpu_step.py (LOSS_RTOL)


def _run(logits, Y, bt, btu, K, w=W):
    """logits [2][n][K] (device), Y [bt] -> (scalars[16], dlogits [2][n][K], pseudo [2][btu]) from the library"""
    lib = _lib.load()
    shape = _lib.Shape(103, 11, 11, 103, K)
    hp = _lib.HParams(5e-4, 0.9, 0.999, 1e-8, 0.3, 0.95, 0.5, 0.8, 0.5, w, 0.8, 0.3)
    n = bt + btu
    ws_bytes = lib.cmlpl_cps_loss_workspace_bytes(C.byref(shape), bt, btu)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV).fill_(0xA5)        # (the call must not rely on zeros)
    scal = torch.full((16,), float("nan"), device=DEV)
    dl = torch.full((2, n, K), float("nan"), device=DEV)
    ps = torch.full((2, btu), -7, dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check("cmlpl_cps_loss_fwd_bwd", lib.cmlpl_cps_loss_fwd_bwd(
        C.byref(shape), bt, btu, p(logits), p(Y), C.byref(hp), p(scal), p(dl), p(ps), p(ws), ws_bytes, st))
    torch.cuda.synchronize()
    return scal.cpu(), dl.cpu(), ps.cpu()


def _torch_ref(logits, Y, bt, w=W):
    """trian_CPS.py:234-250 on CPU in float64 (autograd for the logit gradients)"""
    z = logits.double().clone().requires_grad_(True)
    zs, zw = z[0], z[1]
    cls_s, cls_w = F.cross_entropy(zs[:bt], Y), F.cross_entropy(zw[:bt], Y)                     # :234-235
    t_w = torch.max(logits[0, bt:], 1)[1]                                                       # :238 (fp32, as given)
    t_s = torch.max(logits[1, bt:], 1)[1]                                                       # :239
    con_s, con_w = F.cross_entropy(zs[bt:], t_s), F.cross_entropy(zw[bt:], t_w)                 # :241-244
    total_s, total_w = cls_s + w * con_s, cls_w + w * con_w                                     # :245,248
    (total_s + total_w).backward()
    acc = (torch.max(logits[1, :bt], 1)[1] == Y).float().mean()                                 # :258
    sc = [0.0, total_s, cls_s, con_s, acc, total_w, cls_w, con_w, 0.0, logits.shape[1] - bt, logits.shape[1] - bt, 0.0, 0.0,
          int((t_s == t_w).sum()), 0.0, 0.0]
    return [float(torch.as_tensor(v).detach()) for v in sc], z.grad, torch.stack([t_s, t_w])


def _separated_logits(n, K, g):
    """random logits whose top two entries of every row are at least 1e-3 apart (the argmax is then not a matter of rounding)"""
    z = torch.randn(2, n, K, generator=g) * 2.0
    if K > 1:
        top = torch.topk(z, 2, dim=2)
        close = (top.values[..., 0] - top.values[..., 1]) < 1e-3
        z.scatter_add_(2, top.indices[..., :1], close.unsqueeze(-1).float() * 0.01)
    return z


@pytest.mark.parametrize("K", [9, 15, 16, 64])
@pytest.mark.parametrize("bt,btu", [(128, 128), (64, 512), (8, 8), (1, 1)])
def test_cps_loss_block_matches_torch(K, bt, btu):
    g = torch.Generator().manual_seed(100 * K + bt + btu)
    n = bt + btu
    logits = _separated_logits(n, K, g)
    Y = torch.randint(0, K, (bt,), generator=g)
    sc, dl, ps = _run(logits.to(DEV).contiguous(), Y.to(DEV), bt, btu, K)
    want_sc, want_dl, want_ps = _torch_ref(logits, Y, bt)
    print(f"K={K} {bt}+{btu}: hip={sc[:8].tolist()} torch={want_sc[:8]} agree={sc[13].item()}/{want_sc[13]}")
    assert torch.equal(ps, want_ps)                                              # pseudo-labels exactly
    assert sc[13].item() == want_sc[13] and float(sc[13]) == int(sc[13])         # the agreement count, an integer
    got = np.asarray(sc, np.float64); want = np.asarray(want_sc)
    assert np.all(np.abs(got - want) <= HIST_RTOL * np.abs(want) + 1e-7), (got, want)
    assert [got[i] for i in (0, 8, 11, 12, 14, 15)] == [0.0] * 6 and got[9] == got[10] == btu
    report("dlogits", dl, want_dl, 5e-4, 5e-5 * float(want_dl.abs().max()))
    # Rows of d(loss)/d(logits) sum to zero: (softmax - onehot) * scale.  The computed exponentials are the same numbers
    # in numerator and denominator, so their errors cancel in the row sum; what is left is the rounding of the 6-level
    # sum of exponentials (6 * 2^-24 relative, common to the row) and of the division, the subtraction and the scaling
    # of each of the K stored elements (3 roundings of half an ulp on values <= 1): |sum| <= scale (8 + 2 K) 2^-24.
    rs = dl.double().sum(2).abs()
    scale = torch.cat([torch.full((bt,), 1.0 / bt), torch.full((btu,), W / btu)]).double()
    assert (rs <= scale * (8 + 2 * K) * 2.0 ** -24).all(), float((rs / scale).max())


def test_a_tie_takes_the_first_maximum_and_a_nan_follows_torch_max():
    K, bt, btu = 9, 4, 6
    g = torch.Generator().manual_seed(5)
    logits = _separated_logits(bt + btu, K, g)
    logits[0, bt + 0, 2] = logits[0, bt + 0, 6] = 9.0          # tie in Base's row 0: classes 2 and 6 -> 2
    logits[1, bt + 1, 8] = logits[1, bt + 1, 0] = 7.5          # tie in Base1's row 1: classes 0 and 8 -> 0
    logits[1, bt + 2, :] = 1.25                                # all equal -> 0
    logits[0, 1, 3] = logits[0, 1, 5] = 11.0                   # tie in a LABELLED row of Base (no accuracy there)
    logits[1, 2, 4] = logits[1, 2, 7] = 11.0                   # tie in a labelled row of Base1: accuracy takes class 4
    Y = torch.tensor([0, 3, 4, 1])
    sc, dl, ps = _run(logits.to(DEV).contiguous(), Y.to(DEV), bt, btu, K)
    want_sc, want_dl, want_ps = _torch_ref(logits, Y, bt)
    assert torch.equal(ps, want_ps)
    assert ps[1, 0] == 2 and ps[0, 1] == 0 and ps[0, 2] == 0
    assert sc[13].item() == want_sc[13] and abs(sc[4].item() - want_sc[4]) < 1e-7
    report("dlogits (ties)", dl, want_dl, 5e-4, 5e-5 * float(want_dl.abs().max()))
    # NaN: the maximum for torch.max, and the first NaN of a row wins
    nan = float("nan")
    logits[0, bt + 3, 5] = nan
    logits[0, bt + 3, 7] = nan                                 # Base's row 3: first NaN at class 5
    logits[1, bt + 4, 8] = nan                                 # Base1's row 4: class 8, although 100 is larger than all finite
    logits[1, bt + 4, 1] = 100.0
    sc, dl, ps = _run(logits.to(DEV).contiguous(), Y.to(DEV), bt, btu, K)
    t_w = torch.max(logits[0, bt:], 1)[1]
    t_s = torch.max(logits[1, bt:], 1)[1]
    assert t_w[3] == 5 and t_s[4] == 8                         # (torch's own rule, stated)
    assert torch.equal(ps, torch.stack([t_s, t_w]))
    assert sc[13].item() == int((t_s == t_w).sum())
    _, want_dl, _ = _torch_ref(logits, Y, bt)
    assert torch.equal(torch.isnan(dl), torch.isnan(want_dl.float()))       # NaN lands on the rows torch puts it on
    assert torch.isnan(sc[3]) and torch.isnan(sc[7]) and torch.isfinite(sc[2]) and torch.isfinite(sc[6])


@pytest.mark.parametrize("K,bt,btu", [(9, 128, 128), (16, 64, 512)])
def test_two_runs_give_the_same_bytes(K, bt, btu):
    g = torch.Generator().manual_seed(9)
    logits = _separated_logits(bt + btu, K, g).to(DEV).contiguous()
    Y = torch.randint(0, K, (bt,), generator=g).to(DEV)
    a = _run(logits, Y, bt, btu, K)
    for _ in range(3):
        b = _run(logits, Y, bt, btu, K)
        for x, y in zip(a, b):
            assert x.numpy().tobytes() == y.numpy().tobytes()


def test_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    shape = _lib.Shape(103, 11, 11, 103, 9)
    hp = _lib.HParams()
    t = torch.zeros(4096, device=DEV)
    p = C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.cmlpl_cps_loss_fwd_bwd(C.byref(shape), 0, 8, p, p, C.byref(hp), p, p, p, p, 1 << 14, st) == -1
    assert lib.cmlpl_cps_loss_fwd_bwd(C.byref(shape), 8, 8, p, p, C.byref(hp), p, p, None, p, 1 << 14, st) == -1
    assert lib.cmlpl_cps_loss_fwd_bwd(C.byref(shape), 8, 8, p, p, C.byref(hp), p, p, p, p, 16, st) == -3
    bad = _lib.Shape(103, 11, 11, 103, 65)
    assert lib.cmlpl_cps_loss_fwd_bwd(C.byref(bad), 8, 8, p, p, C.byref(hp), p, p, p, p, 1 << 14, st) == -2
    torch.cuda.synchronize()
