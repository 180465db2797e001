"""GPU: every planner regime of the network kernels against the fp64 oracle, across the accepted shape envelope
(1 <= C <= 256, windows of 4 x 4 up to 20 x 20 -- square or not --, 1 <= K <= 64, bands >= 1: make_dims in api.hip).

One host function, route_net (conv3x3.hip), reads (C, H, W, K, rows) and the switches and decides which kernels run;
conv0a_ok and spe_fused_ok add what depends on the call's arguments.  Each case (tests/envelope_cases.py; the route
itself is held to the same table without a device by tests/test_route_cpu.py) is there for ONE regime and says
which: the forward and the backward run inside cmlpl_timing_begin / _end and the launches per kernel family must be
the regime's signature, and the general 3x3 planner is asked for its plan (cmlpl_debug_conv3_plan) -- a planner change
cannot move a case onto a path another case already covers without this file noticing.

Forward signatures over (conv0_fwd, conv1_fwd, conv2_fwd, head_fwd):
  A  whole-sample kernel (conv0 .. head in one launch)       0 1 0 0
  B  fused conv0 + conv1, general conv2, general head         0 1 1 1
  C  general: one launch per stage                            1 1 1 1
Backward signatures over (head_bwd, conv2_dgrad, conv1_dgrad, conv0_wgrad):
  A  fused head: the data-gradient chain in one launch        0 0 1 0
  B  fused conv1 data gradient + conv0 weight gradient only   1 1 1 0
  C  general                                                  1 1 1 1
(always: one spe_fwd launch -- the nn.Module path takes launch_spe_fwd whatever `bands` is; the step's own choice,
spe_fused_ok, is `test_step_with_more_than_256_bands_takes_the_unfused_spectral_launch` --, one conv1_wgrad entry for
both 3x3 weight gradients, one conv1_wred for the reduce.)

The reference is the oracle in fp64 with the device's ReLU decisions (audited: at most 4 flips, all at |z| < 2e-5);
every output and every live gradient within 2e-6 of its tensor's largest reference element, the bound of
test_split_bf16_convolutions_keep_fp32_accuracy.  The fp32 oracle's own distance from fp64 on the same inputs and gates
is printed next to the device's; a case whose fp32 oracle is itself further than that would get 4 x the oracle's
measured error (docs/EXPERIMENTS.md, "Shape envelope") -- none needs it.

The same cases run again under forced planner switches from tests/test_gpu_env_paths.py; the expected signature
follows the switches (`_under_switches`)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.envelope_cases import CASES, _forced_s, _under_switches
from tests.gpu_util import DEV, ModuleRegions, hip_relu_gates, relu_mask_audit

pytestmark = pytest.mark.gpu

FWD_SIG = {"A": (0, 1, 0, 0), "B": (0, 1, 1, 1), "C": (1, 1, 1, 1)}
BWD_SIG = {"A": (0, 0, 1, 0), "B": (1, 1, 1, 0), "C": (1, 1, 1, 1)}
FWD_IDS = ("conv0_fwd", "conv1_fwd", "conv2_fwd", "head_fwd")
BWD_IDS = ("head_bwd", "conv2_dgrad", "conv1_dgrad", "conv0_wgrad")
BOUND = 2e-6


def _module(shape, params, dropout):
    from cmlpl_amd.models import BaseNet2
    net = BaseNet2(num_features=shape.bands, dropout=dropout, num_classes=shape.K, in_channels=shape.C,
                   window=(shape.H, shape.W)).to(DEV)
    net.load_state_dict(params)
    return net


def _inputs(case):
    shape = O.NetShape(*case.shape)
    n = case.n
    g = torch.Generator().manual_seed(100 + n + 31 * shape.C + 7 * shape.H + shape.W)
    x = torch.randn(n, shape.C, shape.H, shape.W, generator=g)
    y = torch.randn(n, shape.bands, generator=g)
    dm = (torch.rand(n, shape.cls_in, generator=g) < 0.2).float() / 0.2
    dlog = torch.randn(n, shape.K, generator=g)
    dfe = torch.randn(n, 1024, generator=g) * 0.1
    return shape, O.closed_form_params(shape, 7), x, y, dm, dlog, dfe


def _oracle(params, x, y, dm, dlog, dfe, gates, dtype, taps=None):
    """outputs and live gradients of the oracle in `dtype` with the given ReLU decisions"""
    c = lambda t: t.to(dtype)
    pr = {k: c(v).clone().requires_grad_(k in O.LIVE_KEYS) for k, v in params.items()}
    lo, fe = O.basenet2_forward(pr, c(x), c(y), c(dm), taps=taps, relu_gates=gates)
    (lo * c(dlog)).sum().add((fe * c(dfe)).sum()).backward()
    out = {"logits": lo.detach(), "feat": fe.detach()}
    out.update({"grad " + k: pr[k].grad for k in O.LIVE_KEYS})
    return out


@contextlib.contextmanager
def _launch_counts(out):
    """launches per kernel family of the library calls inside (timing state is process-global: always ended)"""
    from cmlpl_amd import _lib
    lib = _lib.load()
    nk = len(_lib.KERNEL_NAMES)
    ms, cnt = (C.c_double * nk)(), (C.c_int64 * nk)()
    _lib.check("cmlpl_timing_begin", lib.cmlpl_timing_begin(0xFFFFFFFF, 64))
    try:
        yield
    finally:
        rc = lib.cmlpl_timing_end(ms, cnt)
    _lib.check("cmlpl_timing_end", rc)
    out.update({k: int(cnt[i]) for i, k in enumerate(_lib.KERNEL_NAMES)})


def _plans(shape, n):
    from cmlpl_amd import _lib
    lib = _lib.load()
    cs = _lib.Shape(shape.C, shape.H, shape.W, shape.bands, shape.K)
    got = []
    for mp, mode in ((0, 0), (0, 1), (1, 0), (1, 1)):
        o = (C.c_int * 3)()
        _lib.check("cmlpl_debug_conv3_plan", lib.cmlpl_debug_conv3_plan(C.byref(cs), 1, n, mp, mode, o))
        got.append(tuple(o))
    return tuple(got)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_forward_backward_against_the_fp64_oracle_in_its_regime(case):
    shape, params, x, y, dm, dlog, dfe = _inputs(case)
    n = case.n
    fwd, bwd, force_s = _under_switches(case)
    plans = _plans(shape, n)
    if force_s:
        assert tuple(p[0] for p in plans) == _forced_s(case, force_s), plans
    else:
        assert plans == case.plans, plans
    net = _module(shape, params, dropout=0.8)
    net.train()
    fc, bc = {}, {}
    with _launch_counts(fc):
        lo, fe = net(x.to(DEV), y.to(DEV), dropmask=dm.to(DEV))
        torch.cuda.synchronize()
    regions = ModuleRegions(net, lo, n)
    gates = hip_relu_gates(regions, shape, n)[0]
    with _launch_counts(bc):
        ((lo * dlog.to(DEV)).sum() + (fe * dfe.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
    sig_f, sig_b = tuple(fc[k] for k in FWD_IDS), tuple(bc[k] for k in BWD_IDS)
    print(f"[{case.id}] {case.why}: forward {sig_f} backward {sig_b} plans {plans}")
    assert sig_f == FWD_SIG[fwd] and fc["spe_fwd"] == 1, (fwd, fc)
    assert sig_b == BWD_SIG[bwd] and bc["conv1_wgrad"] == 1 and bc["conv1_wred"] == 1, (bwd, bc)
    # the oracle in fp64 with the device's ReLU decisions; the decisions audited against its pre-activations
    taps = {}
    ref = _oracle(params, x, y, dm, dlog, dfe, gates, torch.float64, taps)
    flips = relu_mask_audit(regions, [taps], shape, n)[0]
    assert sum(flips.values()) <= 4, flips
    ref32 = _oracle(params, x, y, dm, dlog, dfe, gates, torch.float32)
    hip = dict(net.named_parameters())
    got = {"logits": lo, "feat": fe}
    got.update({"grad " + k: hip[k].grad for k in O.LIVE_KEYS})

    def rel(a, b):
        return float((a.detach().cpu().double() - b).abs().max() / b.abs().max())
    errs = {k: rel(got[k], ref[k]) for k in ref}
    own = {k: rel(ref32[k], ref[k]) for k in ref}
    print({k: f"{v:.2e} (fp32 oracle {own[k]:.2e})" for k, v in errs.items()}, "flips", flips)
    assert all(np.isfinite(v) for v in errs.values()) and max(errs.values()) < BOUND, errs
    for k in ("feat_ss.weight", "feat_ss2.bias", "feat_ss3.weight"):
        assert hip[k].grad is None


def test_regimes_are_each_covered_twice():
    """the table itself: every forward and every backward signature in at least two of its cases"""
    table = [c for c in CASES if c.tag == "table"]
    for r in "ABC":
        assert sum(c.fwd == r for c in table) >= 2 and sum(c.bwd == r for c in table) >= 2, r


def test_inference_and_the_cube_fed_step_refuse_a_non_square_window():
    """BaseNet2 takes an (H, W) pair for the training forward / backward; whole-image inference and the cube-fed step
    stay square-only and must say CMLPL_E_SHAPE, not run"""
    from cmlpl_amd import _lib
    from cmlpl_amd.infer import infer_cube, infer_fused, infer_supported
    lib = _lib.load()
    shape = O.NetShape(6, 9, 11, 5, 3)
    assert not infer_fused(shape) and not infer_supported(shape)
    net = _module(shape, O.closed_form_params(shape, 1), dropout=0.0)
    net.eval()
    assert net.shape.H == 9 and net.shape.W == 11
    cube = torch.zeros(16, 16, shape.C, device=DEV)
    spectra = torch.zeros(256, shape.bands, device=DEV)
    with pytest.raises(_lib.CmlplError) as e:
        infer_cube(net, cube, spectra)
    assert e.value.rc == -2
    flat, packed = net._flat_params(net._live_params())
    labels = torch.zeros(256, dtype=torch.int64, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.cmlpl_infer_cube(C.byref(net._cshape), flat.data_ptr(), packed.data_ptr(), cube.data_ptr(), 16, 16,
                                spectra.data_ptr(), 0, 256, labels.data_ptr(), None, ws.data_ptr(), ws.numel(), st) == -2
    pix = torch.arange(256, dtype=torch.int64, device=DEV)
    assert lib.cmlpl_infer_pixels(C.byref(net._cshape), 1, flat.data_ptr(), flat.numel(), packed.data_ptr(), packed.numel(),
                                  cube.data_ptr(), 16, 16, spectra.data_ptr(), None, pix.data_ptr(), 256,
                                  labels.data_ptr(), None, ws.data_ptr(), ws.numel(), st) == -2
    # the cube-fed step: cmlpl_forward with a scene instead of window tensors
    hp = O.HyperParams()
    chp = _lib.HParams(hp.lr, hp.beta1, hp.beta2, hp.eps, hp.temperature, hp.alpha, hp.noise, hp.dropout,
                       hp.w_contrast, hp.w_mutual, hp.pos_thr, hp.neg_thr)
    b = _lib.Batch()
    xl = torch.zeros(4, shape.bands, device=DEV)
    lp = torch.arange(4, dtype=torch.int64, device=DEV)
    b.d_xl = xl.data_ptr(); b.d_xu = xl.data_ptr(); b.bt = 4; b.btu = 4
    b.d_cube = cube.data_ptr(); b.cube_rows = 16; b.cube_cols = 16; b.d_lab_pix = lp.data_ptr(); b.d_unl_pix = lp.data_ptr()
    params2 = torch.zeros(2, flat.numel(), device=DEV)
    packed2 = torch.zeros(2, packed.numel(), device=DEV)
    logits = torch.zeros(2, 8, shape.K, device=DEV)
    feat = torch.zeros(2, 8, 1024, device=DEV)
    need = lib.cmlpl_workspace_bytes(C.byref(net._cshape), 2, 8, 8)
    assert need > 0                                       # (the split-fed step does take the window)
    ws2 = torch.zeros(need, dtype=torch.uint8, device=DEV)
    rc = lib.cmlpl_forward(C.byref(net._cshape), C.byref(chp), C.byref(b), None, params2.data_ptr(), packed2.data_ptr(),
                           None, 1, 0, 0, logits.data_ptr(), feat.data_ptr(), None, ws2.data_ptr(), ws2.numel(), st)
    assert rc == -2, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("bands,augment", [(256, 0), (300, 1)])
def test_step_with_more_than_256_bands_takes_the_unfused_spectral_launch(bands, augment):
    """spe_fused_ok: up to 256 bands the step's spectral branch is ONE launch that augments the raw spectra in registers;
    beyond, the augmentation kernel writes the augmented spectra and launch_spe_fwd reads them (the path every other test
    reaches through CMLPL_FUSE_SPE=0 only).  40 channels on 8 x 8 windows: both convolution passes are fused, so the
    augmentation launch is there for the spectra alone -- 0 launches at 256 bands, 1 at 300.  Two steps (the second on
    weights the first one's feat_spe gradient moved) against the oracle, loss rows within 1e-4 relative."""
    from cmlpl_amd import HyperParams, NetShape, TrainEngine
    shape = O.NetShape(40, 8, 8, bands, 5)
    hp = O.HyperParams()
    bt = btu = 8
    p0, p1 = O.closed_form_params(shape, 1), O.closed_form_params(shape, 2)
    st = O.StepState.create(shape, p0, p1, bt, hp)
    eng = TrainEngine(NetShape(shape.C, shape.H, shape.W, shape.bands, shape.K), bt, btu, HyperParams(), device=DEV)
    eng.load_state_dict(0, p0)
    eng.load_state_dict(1, p1)
    d = lambda t: t.to(DEV)
    for s in range(2):
        b = O.synthetic_batch(shape, bt, btu, 700 + s)
        cnt = {}
        with _launch_counts(cnt):
            eng.step(d(b["XPl"]), d(b["Xl"]), d(b["Y"]), d(b["XPu"]), d(b["Xu"]), 1, s,
                     noise=[d(t) for t in b["noise"]], dropmask=torch.stack(b["dropmask"]).to(DEV))
            torch.cuda.synchronize()
        gates = hip_relu_gates(eng, shape, bt + btu)
        ref = O.train_step(st, b["XPl"], b["Xl"], b["Y"], b["XPu"], b["Xu"], b["noise"], b["dropmask"], 1, s, hp,
                           relu_gates=gates)
        row = eng.loss_row()
        print(f"[{bands} bands] step {s}: hip={row} oracle={ref['hist']} augment launches {cnt['augment']} spe_fwd {cnt['spe_fwd']}")
        assert cnt["augment"] == augment and cnt["spe_fwd"] == 1, cnt
        assert (cnt["conv0_fwd"], cnt["conv1_fwd"], cnt["conv2_fwd"], cnt["head_fwd"]) == FWD_SIG["A"], cnt
        for got, want in zip(row, ref["hist"]):
            assert abs(got - want) <= 1e-4 * abs(want) + 1e-6, (s, row, ref["hist"])
