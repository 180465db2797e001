"""GPU: the gradient norm, the clip coefficient and the clipped, decayed Adam step against their definitions in numpy
(cmlpl_amd/optim.py; include/cmlpl.h, "THE DEFINITION OF A CLIPPED, DECAYED ADAM STEP"), and the whole step with a
schedule, decay and clipping: eager against replayed, bit for bit.

Tolerances.  The norm: 1 ulp of fp32 -- the fp64 sum of ~2e5 exact products is off by at most ~2^-35 relative whatever
the order, far under half an fp32 ulp, so only the final rounding can differ.  The coefficient: bit-equal to the fp32
chain on the kernel's own norm.  The update: rtol 1e-6 / atol 1e-7, what tests/test_gpu_ops.py holds plain Adam to.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from cmlpl_amd import HyperParams, NetShape, TrainEngine, _lib
from cmlpl_amd.optim import (LRSchedule, OptimConfig, adamw_host, clip_coef_host, grad_norm_host, live_ranges)
from cmlpl_amd.patches import extract_patches
from tests.gpu_util import DEV, report

pytestmark = pytest.mark.gpu

SHAPES = {"W12": (5, 12, 12, 9, 3),          # K = 3: one pad float behind classifier.bias
          "B2": (103, 11, 11, 103, 9)}       # K = 9: three
BT = BTU = 8


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Net:
    """layout, hyper-parameters and the partials / norms buffers of one shape"""

    def __init__(self, name):
        self.lib = _lib.load()
        self.cs = _lib.Shape(*SHAPES[name])
        self.L = _lib.layout(self.cs)
        self.P, self.live, self.PK = int(self.L.param_total), int(self.L.param_live), int(self.L.packed_total)
        self.ranges = live_ranges(self.L.param_off, self.L.param_numel)
        h = HyperParams()
        self.hp = h
        self.chp = _lib.HParams(h.lr, h.beta1, h.beta2, h.eps, h.temperature, h.alpha, h.noise, h.dropout,
                                h.w_contrast, h.w_mutual, h.pos_thr, h.neg_thr)
        self.partials = torch.empty(self.lib.cmlpl_grad_norm_partials_bytes() // 8, dtype=torch.float64, device=DEV)

    def live_mask(self, stride):
        m = np.zeros(stride, bool)
        for off, n in self.ranges:
            m[off:off + n] = True
        return m

    def grad_norm(self, grads, nets, stride, max_norm):
        """the norms row of one cmlpl_grad_norm call (slots it does not write stay -7)"""
        norms = torch.full((4,), -7.0, device=DEV)
        self.partials.fill_(float("nan"))            # (the workspace needs no initialisation)
        rc = self.lib.cmlpl_grad_norm(C.byref(self.cs), nets, grads.data_ptr(), stride, max_norm, self.partials.data_ptr(),
                                      norms.data_ptr(), _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return norms.cpu().numpy()


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def _poison(g, mask):
    """every float outside the live tensors: 1e30 and NaN in turn"""
    idx = np.nonzero(~mask)[0]
    g[:, idx[0::2]] = 1e30
    g[:, idx[1::2]] = np.nan
    return g


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("nets,extra", [(1, 0), (2, 0), (2, 12)])
def test_grad_norm_matches_the_fp64_definition(name, nets, extra):
    net = Net(name)
    stride = net.P + extra
    mask = net.live_mask(stride)
    assert (~mask[:net.live]).sum() == (-SHAPES[name][4]) % 4        # the pad floats behind classifier.bias
    rng = np.random.default_rng(3)
    g = _poison((rng.standard_normal((nets, stride)) * 0.3).astype(np.float32), mask)
    dg = torch.from_numpy(g).to(DEV)
    max_norm = 1.0
    row = net.grad_norm(dg, nets, stride, max_norm)
    again = net.grad_norm(dg, nets, stride, max_norm)
    assert row.tobytes() == again.tobytes()                            # the same bytes on every run
    for n in range(nets):
        S, want = grad_norm_host(g[n], net.L.param_off, net.L.param_numel)
        print(f"[{name} nets={nets} stride=+{extra}] net {n}: S={S!r} norm gpu={row[n]!r} host={want!r} coef={row[2 + n]!r}")
        assert np.isfinite(row[n]) and _ulps(row[n], want) <= 1
        assert row[2 + n].tobytes() == clip_coef_host(row[n], max_norm).tobytes() and row[2 + n] < 1.0
    if nets == 1:
        assert row[1] == -7.0 and row[3] == -7.0                       # a call over one network writes slots 0 and 2 only


def test_grad_norm_edge_values():
    net = Net("W12")
    P, mask = net.P, net.live_mask(net.P)
    live_idx = np.nonzero(mask)[0]
    # all-zero gradients: norm 0, coefficient exactly 1
    row = net.grad_norm(torch.zeros(2, P, device=DEV), 2, P, 1.0)
    assert row.tolist() == [0.0, 0.0, 1.0, 1.0]
    # entries whose fp32 squares would overflow (1e25) or vanish (1e-30)
    g = np.zeros((2, P), np.float32)
    g[0, live_idx[[3, 500, -1]]] = 1e25
    g[1, live_idx[::7]] = 1e-30
    row = net.grad_norm(torch.from_numpy(g).to(DEV), 2, P, 1.0)
    for n in range(2):
        S, want = grad_norm_host(g[n], net.L.param_off, net.L.param_numel)
        print(f"extremes net {n}: S={S!r} gpu={row[n]!r} host={want!r}")
        assert want > 0 and np.isfinite(want) and _ulps(row[n], want) <= 1
        assert row[2 + n].tobytes() == clip_coef_host(row[n], 1.0).tobytes()
    assert row[2] < 1e-24 and row[3] == 1.0
    # max_norm == 0: no clipping, whatever the norm
    row0 = net.grad_norm(torch.from_numpy(g).to(DEV), 2, P, 0.0)
    assert row0[:2].tobytes() == row[:2].tobytes() and row0[2:].tolist() == [1.0, 1.0]
    # one NaN in a live tensor of network 1 only
    rng = np.random.default_rng(5)
    g = rng.standard_normal((2, P)).astype(np.float32)
    clean = net.grad_norm(torch.from_numpy(g).to(DEV), 2, P, 1.0)
    g[1, live_idx[len(live_idx) // 2]] = np.nan
    row = net.grad_norm(torch.from_numpy(g).to(DEV), 2, P, 1.0)
    assert np.isnan(row[1]) and np.isnan(row[3])
    assert row[0].tobytes() == clean[0].tobytes() and row[2].tobytes() == clean[2].tobytes()
    assert np.isnan(clip_coef_host(np.float32("nan"), 1.0))


def _adam_opt(net, p, g, m, v, t, packed, opt):
    rc = net.lib.cmlpl_adam_step_opt(C.byref(net.cs), 2, p.data_ptr(), net.P, g.data_ptr(), net.P, m.data_ptr(), v.data_ptr(),
                                     t, C.byref(net.chp), None if packed is None else packed.data_ptr(),
                                     None if opt is None else C.byref(opt), _stream())
    assert rc == 0, rc


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_adam_step_opt_matches_adamw_host_and_keeps_the_packed_copies(name):
    net = Net(name)
    P, PK, st = net.P, net.PK, _stream()
    rng = np.random.default_rng(11)
    p0 = (rng.standard_normal((2, P)) * 0.05).astype(np.float32)
    dp = torch.from_numpy(p0).to(DEV)
    dm, dv = torch.zeros(2, P, device=DEV), torch.zeros(2, P, device=DEV)
    packed = torch.full((2, PK), float("nan"), device=DEV)
    assert net.lib.cmlpl_pack_weights(C.byref(net.cs), 2, dp.data_ptr(), P, packed.data_ptr(), st) == 0
    norms = torch.zeros(4, device=DEV)
    wd = 0.05
    hp, hm, hv = p0.copy(), np.zeros((2, P), np.float32), np.zeros((2, P), np.float32)
    h = net.hp
    for t in range(1, 4):
        g = (rng.standard_normal((2, P)) * 0.2 * t).astype(np.float32)
        dg = torch.from_numpy(g).to(DEV)
        # max_norm at half the measured norm of network 0: both networks clip, by about one half
        measured = net.grad_norm(dg, 2, P, 0.0)
        max_norm = float(measured[0]) / 2
        opt = _lib.Optim(max_norm, wd, norms.data_ptr(), net.partials.data_ptr())
        _adam_opt(net, dp, dg, dm, dv, t, packed, opt)
        torch.cuda.synchronize()
        row = norms.cpu().numpy()
        assert row[:2].tobytes() == measured[:2].tobytes()             # the step's fold is cmlpl_grad_norm's
        for n in range(2):
            coef = clip_coef_host(row[n], max_norm)
            assert row[2 + n].tobytes() == coef.tobytes() and 0.4 < coef < 0.6
            for off, k in net.ranges:
                s = slice(off, off + k)
                hp[n, s], hm[n, s], hv[n, s] = adamw_host(hp[n, s], g[n, s], hm[n, s], hv[n, s], t, h.lr, h.beta1, h.beta2,
                                                          h.eps, weight_decay=wd, coef=coef)
        mask = net.live_mask(P)
        report(f"{name} t={t} params", dp[:, mask], hp[:, mask], 1e-6, 1e-7)
        report(f"{name} t={t} m", dm[:, mask], hm[:, mask], 1e-6, 1e-7)
        report(f"{name} t={t} v", dv[:, mask], hv[:, mask], 1e-6, 1e-7)
        assert dp[:, net.live:].cpu().numpy().tobytes() == p0[:, net.live:].tobytes()     # dead tensors: bit-unchanged
    assert float(np.abs(hp - p0).max()) > 1e-4
    want = torch.empty(2, PK, device=DEV)
    assert net.lib.cmlpl_pack_weights(C.byref(net.cs), 2, dp.data_ptr(), P, want.data_ptr(), st) == 0
    torch.cuda.synchronize()
    a, b = packed.view(torch.int32).cpu(), want.view(torch.int32).cpu()
    assert not (a != b).any(), f"{int((a != b).sum())} packed words differ"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_adam_step_opt_with_everything_off_is_adam_step_bit_for_bit(name):
    net = Net(name)
    P, PK, st = net.P, net.PK, _stream()
    rng = np.random.default_rng(2)
    p0 = torch.from_numpy((rng.standard_normal((2, P)) * 0.05).astype(np.float32)).to(DEV)
    state = []
    norms = torch.full((4,), -7.0, device=DEV)
    for opt in (None, _lib.Optim(0.0, 0.0, None, None), _lib.Optim(0.0, 0.0, norms.data_ptr(), net.partials.data_ptr())):
        p, m, v = p0.clone(), torch.zeros(2, P, device=DEV), torch.zeros(2, P, device=DEV)
        packed = torch.zeros(2, PK, device=DEV)
        assert net.lib.cmlpl_pack_weights(C.byref(net.cs), 2, p.data_ptr(), P, packed.data_ptr(), st) == 0
        g = np.random.default_rng(9)
        for t in range(1, 4):
            dg = torch.from_numpy(g.standard_normal((2, P)).astype(np.float32) * 0.1).to(DEV)
            if opt is None:
                rc = net.lib.cmlpl_adam_step(C.byref(net.cs), 2, p.data_ptr(), P, dg.data_ptr(), P, m.data_ptr(), v.data_ptr(),
                                             t, C.byref(net.chp), packed.data_ptr(), st)
                assert rc == 0, rc
            else:
                _adam_opt(net, p, dg, m, v, t, packed, opt)
        torch.cuda.synchronize()
        state.append([x.cpu().numpy().tobytes() for x in (p, m, v, packed)])
    assert state[0] == state[1] and state[0] == state[2]
    row = norms.cpu().numpy()
    assert row[0] > 0 and row[1] > 0 and row[2:].tolist() == [1.0, 1.0]       # the row is written without clipping too


def test_options_are_checked_before_any_launch():
    net = Net("W12")
    P = net.P
    p, g, m, v = (torch.zeros(2, P, device=DEV) for _ in range(4))
    norms = torch.zeros(4, device=DEV)

    def rc(opt, chp=net.chp):
        return net.lib.cmlpl_adam_step_opt(C.byref(net.cs), 2, p.data_ptr(), P, g.data_ptr(), P, m.data_ptr(), v.data_ptr(), 1,
                                           C.byref(chp), None, C.byref(opt), _stream())
    part = net.partials.data_ptr()
    assert rc(_lib.Optim(-1.0, 0.0, None, part)) == -1
    assert rc(_lib.Optim(float("nan"), 0.0, None, part)) == -1
    assert rc(_lib.Optim(0.0, float("inf"), None, part)) == -1
    assert rc(_lib.Optim(1.0, 0.0, None, None)) == -1                  # clipping without the partials
    assert rc(_lib.Optim(0.0, 0.0, norms.data_ptr(), None)) == -1      # the row without the partials
    one = _lib.HParams.from_buffer_copy(net.chp)
    one.lr = 0.5
    assert rc(_lib.Optim(0.0, 2.0, None, None), one) == -1             # keep == 0.0f: its bits would say "off"
    a, b, c = C.c_float(), C.c_float(), C.c_float()
    assert net.lib.cmlpl_dyn_adam_opt(C.byref(one), 1, 2.0, C.byref(a), C.byref(b), C.byref(c)) == -1
    assert net.lib.cmlpl_dyn_adam_opt(C.byref(net.chp), 3, 0.05, C.byref(a), C.byref(b), C.byref(c)) == 0
    a0, b0 = C.c_float(), C.c_float()
    assert net.lib.cmlpl_dyn_adam(C.byref(net.chp), 3, C.byref(a0), C.byref(b0)) == 0
    assert (a.value, b.value) == (a0.value, b0.value)
    assert np.float32(c.value).tobytes() == np.float32(1.0 - float(np.float32(net.hp.lr)) * float(np.float32(0.05))).tobytes()
    torch.cuda.synchronize()
    assert not p.any() and not m.any()                                   # nothing was launched


# ------------------------------------------------------------------ the whole step
def _scene(shape, n_lab, n_unl, seed):
    Cc, H, W, bands, K = shape
    rows, cols = H + 9, W + 7
    g = torch.Generator().manual_seed(seed)
    cube = torch.randn(rows, cols, Cc, generator=g)
    lab_pix = torch.randint(0, rows * cols, (n_lab,), generator=g)
    unl_pix = torch.randint(0, rows * cols, (n_unl,), generator=g)
    X = torch.randn(n_lab, bands, generator=g)
    Y = torch.randint(0, K, (n_lab,), generator=g)
    Xu = torch.randn(n_unl, bands, generator=g)
    return [t.to(DEV).contiguous() for t in (cube, lab_pix, unl_pix, X, Y, Xu)]


def _engine(shape, hist_rows=8, **kw):
    eng = TrainEngine(NetShape(*shape), BT, BTU, HyperParams(), device=DEV, seed=1088, hist_rows=hist_rows, **kw)
    eng.init_params_default(1088)
    return eng


def _config(total=6):
    return OptimConfig(schedule=LRSchedule("cosine", 5e-4, total, warmup_steps=2, lr_min=1e-5), weight_decay=0.05,
                       clip_grad=0.5)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_step_without_update_leaves_gradients_whose_norm_is_the_written_row(name):
    shape = SHAPES[name]
    cube, lab_pix, unl_pix, X, Y, Xu = _scene(shape, BT, BTU, 4)
    XP, XPu = extract_patches(cube, lab_pix, shape[1]), extract_patches(cube, unl_pix, shape[1])
    eng = _engine(shape, optim=_config())
    before = eng.params.clone()
    eng.step(XP, X, Y, XPu, Xu, 0, 0, apply_update=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, before) and eng.adam_t == 0
    row = np.asarray(eng.grad_norms(), np.float32)
    g = eng.grads.cpu().numpy()
    for n in range(2):
        S, want = grad_norm_host(g[n], eng.layout.param_off, eng.layout.param_numel)
        print(f"[{name}] net {n}: norm gpu={row[n]!r} host={want!r} coef={row[2 + n]!r}")
        assert want > 0 and _ulps(row[n], want) <= 1
        assert row[2 + n].tobytes() == clip_coef_host(row[n], 0.5).tobytes()


@pytest.mark.parametrize("method", ["cmlpl", "cps"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_six_scheduled_steps_eager_and_replayed_are_the_same_bytes(name, method):
    shape = SHAPES[name]
    cube, lab_pix, unl_pix, X, Y, Xu = _scene(shape, 4 * BT + 5, 4 * BTU + 3, 11)
    XP, XPu = extract_patches(cube, lab_pix, shape[1]), extract_patches(cube, unl_pix, shape[1])
    g = torch.Generator().manual_seed(5)
    lab_perm = torch.randperm(X.shape[0], generator=g).to(DEV)
    unl_perm = torch.randperm(Xu.shape[0], generator=g).to(DEV)
    steps = 7                                    # one eager step in front of the capture, then programs of 3 + 3
    cfg = _config(total=steps)
    offs = [(k % 4) * BT for k in range(steps)], [(k % 4) * BTU for k in range(steps)]
    ea, eb = _engine(shape, method=method, optim=cfg), _engine(shape, method=method, optim=cfg)
    for k in range(steps):
        ea.step(XP, X, Y, XPu, Xu, k // 4, k % 4, lab_idx=lab_perm[offs[0][k]:offs[0][k] + BT],
                unl_idx=unl_perm[offs[1][k]:offs[1][k] + BTU])
    eb.step(XP, X, Y, XPu, Xu, 0, 0, lab_idx=lab_perm[:BT], unl_idx=unl_perm[:BTU])
    graph = eb.capture(XP, X, Y, XPu, Xu, lab_perm, unl_perm, BT, BTU, capacity=8)
    for lo in (1, 4):
        graph.program([(k // 4, k % 4, offs[0][k], offs[1][k]) for k in range(lo, lo + 3)])
        for _ in range(3):
            graph.launch()
    torch.cuda.synchronize()
    assert ea.adam_t == eb.adam_t == steps
    for what, a, b in (("params", ea.params, eb.params), ("m", ea.m, eb.m), ("v", ea.v, eb.v),
                       ("norms ring", ea.norm_hist, eb.norm_hist), ("scalars ring", ea.scalar_hist, eb.scalar_hist)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"{name} {method}: {what} differ"
    ring = ea.norm_window(steps)
    print(f"[{name} {method}] norms ring:\n{ring}")
    assert np.isfinite(ring).all() and (ring[:, :2] > 0).all() and (ring[:, 2:] <= 1).all()
    assert ea.grad_norms() == ring[-1].tolist()
    # the schedule has been at work: the engine without one is somewhere else
    assert [ea.lr_of(t) for t in (1, 2, 3)] == [float(np.float32(cfg.schedule.lr_at(t))) for t in (1, 2, 3)]
    assert ea.lr_of(1) == float(np.float32(2.5e-4)) and ea.lr_of(3) == float(np.float32(5e-4))
    graph.close()


def test_cube_fed_scheduled_steps_are_the_split_fed_ones():
    shape = SHAPES["B2"]
    cube, lab_pix, unl_pix, X, Y, Xu = _scene(shape, BT, BTU, 6)
    XP, XPu = extract_patches(cube, lab_pix, shape[1]), extract_patches(cube, unl_pix, shape[1])
    li, ui = torch.arange(BT, device=DEV), torch.arange(BTU, device=DEV)
    ea, eb = _engine(shape, optim=_config()), _engine(shape, optim=_config())
    for s in range(3):
        ea.step(XP, X, Y, XPu, Xu, 0, s, lab_idx=li, unl_idx=ui)
        eb.step(None, X, Y, None, Xu, 0, s, lab_idx=li, unl_idx=ui, cube=cube, lab_pix=lab_pix, unl_pix=unl_pix)
    torch.cuda.synchronize()
    for a, b in ((ea.params, eb.params), (ea.m, eb.m), (ea.norm_hist, eb.norm_hist)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_default_config_is_no_config_and_an_option_changes_the_step():
    shape = SHAPES["B2"]
    cube, lab_pix, unl_pix, X, Y, Xu = _scene(shape, BT, BTU, 2)
    XP, XPu = extract_patches(cube, lab_pix, shape[1]), extract_patches(cube, unl_pix, shape[1])
    ea, eb = _engine(shape, optim=None), _engine(shape, optim=OptimConfig())
    ec = _engine(shape, optim=OptimConfig(weight_decay=0.05, clip_grad=0.01), teacher_alpha=0.9)
    assert eb.optim is None and eb.norm_hist is None and ea.identity() == eb.identity()
    assert "clip_grad" in ec.identity() and "clip_grad" not in ea.identity()
    for s in range(3):
        for e in (ea, eb, ec):
            e.step(XP, X, Y, XPu, Xu, 1, s)
    torch.cuda.synchronize()
    for a, b in ((ea.params, eb.params), (ea.m, eb.m), (ea.v, eb.v), (ea.scalar_hist, eb.scalar_hist),
                 (ea.bank_feats, eb.bank_feats), (ea.packed, eb.packed)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert not torch.equal(ea.params, ec.params)
    row = ec.grad_norms()
    assert row[0] > 0.01 and row[2] < 1.0 and torch.isfinite(ec.teacher_params).all()       # clipped, the teacher follows
    with pytest.raises(RuntimeError):
        ea.grad_norms()


def test_sharded_engine_refuses_the_options():
    from cmlpl_amd.distributed import DistTrainEngine
    with pytest.raises(ValueError, match="optim"):
        DistTrainEngine(NetShape(*SHAPES["B2"]), BT, BTU, HyperParams(), device=DEV, optim=OptimConfig(clip_grad=1.0))
