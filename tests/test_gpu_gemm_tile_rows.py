"""GPU: the row loop of the weight-gradient GEMM tiles (csrc/gemm_tn.hpp: GemmTNWalk, gemm_tn_rows) at its edges.

The classifier and feat_spe weight gradients are two transposed-A GEMMs whose contraction runs over the rows per
network, R = bt + btu.  A tile's four waves take a quarter of the (R + 1) / 2 row pairs each, sixteen pairs to a batch,
two batches requested ahead.  The rows per network of the cases:
  2, 3, 7        waves with no pairs at all (2: waves 1 - 3; 3: waves 2 and 3, and wave 1's only pair is half empty; 7:
                 one pair per wave, the last half empty);
  33             an odd R inside a batch: the last pair is half empty;
  120 .. 136     a wave at 15, 16 and 17 pairs: the batch edge, where the second batch begins;
  248 .. 257     the second batch full (256), then a third batch: the first trip round the two register sets;
  264            33 pairs.
R = 1 cannot be a training step: the C ABI and the engine take bt >= 1 and btu >= 1 (asserted below), so the least
contraction a step's tiles can see is 2; what R = 1 exercises -- a single, half-empty pair with three idle waves -- is
what wave 1 runs at R = 3 there.  R = 1 itself is run through the entry that does reach it: one network's backward
(cmlpl_basenet2_bwd under cmlpl_amd.models.BaseNet2, reduce_gemm_kernel: gemm_tn_block<false>) on a single row, held to
the fp64 oracle at the same bound.
The window is 8 x 8 with C = 5 and bands = 5; M = K = 9 is a ragged M tile.  One more shape has bands = 103: feat_spe's
N tile is ragged (103 = 3 * 32 + 7) and the rows of `sn` are not 16-byte aligned.  The backward route of every case is
asserted (cmlpl_debug_route), as tests/test_gpu_fold_chain.py does.

Each case runs ONE training step through the C ABI twice from the same state -- the default path, asserted by its
launch counts to be the fused fold + Adam launch (gemm_tn_block<true>), and CMLPL_FUSE_ADAM=0 (reduce_gemm_kernel +
adam_kernel: gemm_tn_block<false>) -- and asserts
  1. gradients, parameters, m, v and the packed block are byte-equal between the two paths;
  2. the classifier and feat_spe weight and bias gradients agree with the fp64 oracle at the bound
     tests/test_gpu_step.py holds gradients to.
Both paths run the same row walk (GemmTNWalk / gemm_tn_rows) in two instantiations of gemm_tn_block, so (1) cannot see
a fault the two have in common: what holds the walk itself is (2) -- a dropped or doubled row at these R is far outside
that bound -- and, outside this suite, the byte comparison of the benchmark's outputs with the commit before.  The
segmented instantiation (GemmTN::b_seg_rows > 0) is not run by this file: the sharded-engine tests hold it.
The oracle alone is checked (without a GPU) to give finite, non-zero gradients in those four tensors.
"""
import ctypes as C
import os

import pytest
import torch

from oracle import cmlpl_oracle as O

DEV = "cuda:0"
ROUTE_C = 2
SHAPES = {"w8b5": O.NetShape(5, 8, 8, 5, 9), "w8b103": O.NetShape(5, 8, 8, 103, 9)}
ROWS = (2, 3, 7, 33, 120, 127, 128, 129, 136, 248, 255, 256, 257, 264)
CASES = [("w8b5", n) for n in ROWS] + [("w8b103", 129)]
KEYS = ("classifier.weight", "classifier.bias", "feat_spe.weight", "feat_spe.bias")
FIELDS = ("grads", "params", "m", "v", "packed")
_params = {}


def _split(n):
    return n // 2, n - n // 2


def _state(name):
    if name not in _params:
        _params[name] = (O.closed_form_params(SHAPES[name], 9), O.closed_form_params(SHAPES[name], 10))
    return _params[name]


def _switch(value):
    from cmlpl_amd import _lib
    if value is None:
        os.environ.pop("CMLPL_FUSE_ADAM", None)
    else:
        os.environ["CMLPL_FUSE_ADAM"] = value
    _lib.load().cmlpl_debug_reload_switches()


def _step(name, n, fuse, batch):
    """one step from the common state with CMLPL_FUSE_ADAM = fuse -> (engine, {field: bytes}, launch counts)"""
    from cmlpl_amd import TrainEngine, _lib
    from tests.gpu_util import cuda_batch, to_hp, to_shape
    bt, btu = _split(n)
    old = os.environ.get("CMLPL_FUSE_ADAM")
    _switch(fuse)
    try:
        eng = TrainEngine(to_shape(SHAPES[name]), bt, btu, to_hp(O.HyperParams()), device=DEV)
        for net, p in enumerate(_state(name)):
            eng.load_state_dict(net, {k: v.clone() for k, v in p.items()})
        cb = cuda_batch(batch)
        nk = len(_lib.KERNEL_NAMES)
        ms, cnt = (C.c_double * nk)(), (C.c_int64 * nk)()
        _lib.check("cmlpl_timing_begin", eng.lib.cmlpl_timing_begin(0xFFFFFFFF, 64))
        try:
            eng.step(cb["XPl"], cb["Xl"], cb["Y"], cb["XPu"], cb["Xu"], 1, 0, noise=cb["noise"], dropmask=cb["dropmask"])
        finally:
            rc = eng.lib.cmlpl_timing_end(ms, cnt)
        _lib.check("cmlpl_timing_end", rc)
        counts = {k: int(cnt[i]) for i, k in enumerate(_lib.KERNEL_NAMES)}
        torch.cuda.synchronize()
        got = {"grads": eng.grads, "params": eng.params, "m": eng.m, "v": eng.v, "packed": eng.packed}
        return eng, {k: t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes() for k, t in got.items()}, counts
    finally:
        _switch(old)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_oracle_alone_gives_finite_nonzero_gemm_gradients(name):
    shape = SHAPES[name]
    bt, btu = _split(33)
    p0, p1 = _state(name)
    hp = O.HyperParams()
    st = O.StepState.create(shape, p0, p1, bt, hp)
    b = O.synthetic_batch(shape, bt, btu, 77)
    ref = O.train_step(st, b["XPl"], b["Xl"], b["Y"], b["XPu"], b["Xu"], b["noise"], b["dropmask"], 1, 0, hp)
    for net in range(2):
        for k in KEYS:
            g = ref["grads"][net][k]
            assert torch.isfinite(g).all(), (net, k)
            nz = int((g != 0).sum())
            print(f"[{name}] oracle grad[{net}] {k}: max|g|={float(g.abs().max()):.3e}, {nz}/{g.numel()} non-zero")
            assert nz > g.numel() // 2 and float(g.abs().max()) > 1e-6, (net, k, nz)


@pytest.mark.gpu
def test_a_training_step_has_at_least_two_rows_per_network():
    """R = 1 would be bt = 0 or btu = 0: the engine refuses such a batch, so the tiles never contract over one row"""
    from cmlpl_amd import TrainEngine
    from tests.gpu_util import cuda_batch, to_hp, to_shape
    shape = SHAPES["w8b5"]
    eng = TrainEngine(to_shape(shape), 1, 1, to_hp(O.HyperParams()), device=DEV)
    cb = cuda_batch(O.synthetic_batch(shape, 1, 1, 77))
    with pytest.raises(ValueError):
        eng.step(cb["XPl"][:0], cb["Xl"][:0], cb["Y"][:0], cb["XPu"], cb["Xu"], 1, 0, noise=cb["noise"], dropmask=cb["dropmask"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_row_through_one_networks_backward_meets_the_oracle(name):
    """R = 1: the four GEMM gradients of a single row, against the fp64 oracle with the device's ReLU decisions"""
    from cmlpl_amd.models import BaseNet2
    from tests.gpu_util import ModuleRegions, hip_relu_gates, report
    shape, n = SHAPES[name], 1
    params = _state(name)[0]
    g = torch.Generator().manual_seed(101)
    x = torch.randn(n, shape.C, shape.H, shape.W, generator=g)
    y = torch.randn(n, shape.bands, generator=g)
    dm = (torch.rand(n, shape.cls_in, generator=g) < 0.2).float() / 0.2
    dlog = torch.randn(n, shape.K, generator=g)
    dfe = torch.randn(n, 1024, generator=g) * 0.1
    net = BaseNet2(num_features=shape.bands, dropout=0.8, num_classes=shape.K, in_channels=shape.C, window=shape.H).to(DEV)
    net.load_state_dict(params)
    net.train()
    lo, fe = net(x.to(DEV), y.to(DEV), dropmask=dm.to(DEV))
    gates = hip_relu_gates(ModuleRegions(net, lo, n), shape, n)[0]
    ((lo * dlog.to(DEV)).sum() + (fe * dfe.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    pr = {k: v.clone().double().requires_grad_(k in O.LIVE_KEYS) for k, v in params.items()}
    lo_ref, fe_ref = O.basenet2_forward(pr, x.double(), y.double(), dm.double(), relu_gates=gates)
    (lo_ref * dlog.double()).sum().add((fe_ref * dfe.double()).sum()).backward()
    hip = dict(net.named_parameters())
    for k in KEYS:
        gr = pr[k].grad
        assert torch.isfinite(gr).all() and float(gr.abs().max()) > 1e-6, k        # (not vacuous)
        mx = max(float(gr.abs().max()), 1e-4)
        report(f"[{name} n=1] grad {k}", hip[k].grad, gr, 5e-4, 5e-5 * mx)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", CASES, ids=[f"{a}-{n}" for a, n in CASES])
def test_both_tile_loops_are_byte_equal_and_meet_the_oracle(name, n):
    from cmlpl_amd import _lib
    from tests.gpu_util import hip_relu_gates, report
    shape = SHAPES[name]
    route = (C.c_int * 40)()
    _lib.check("cmlpl_debug_route", _lib.load().cmlpl_debug_route(
        C.byref(_lib.Shape(shape.C, shape.H, shape.W, shape.bands, shape.K)), 2, n, route))
    print(f"[{name} n={n}] backward route {route[1]}")
    assert route[1] == ROUTE_C, f"{name} n={n}: backward route {route[1]}"
    bt, btu = _split(n)
    hp = O.HyperParams()
    b = O.synthetic_batch(shape, bt, btu, 77)
    eng, fused, c_fused = _step(name, n, None, b)
    assert c_fused["conv1_wred"] == 1 and c_fused["adam"] == 0, c_fused      # the fused fold + Adam launch
    # (2) the oracle with the device's ReLU decisions, as tests/test_gpu_step.py compares gradients
    st = O.StepState.create(shape, *_state(name), bt, hp)
    ref = O.train_step(st, b["XPl"], b["Xl"], b["Y"], b["XPu"], b["Xu"], b["noise"], b["dropmask"], 1, 0, hp,
                       relu_gates=hip_relu_gates(eng, shape, n))
    for net in range(2):
        for k in KEYS:
            gr = ref["grads"][net][k]
            mx = max(float(gr.abs().max()), 1e-4)
            report(f"[{name} n={n}] grad[{net}] {k}", eng.grad(net, k), gr, 5e-4, 5e-5 * mx)
    del eng
    # (1) the two launches it replaces
    _, two, c_two = _step(name, n, "0", b)
    assert c_two["conv1_wred"] == 1 and c_two["adam"] >= 1, c_two
    for f in FIELDS:
        assert fused[f] == two[f], f"{name} n={n}: `{f}` differs between the fused launch and CMLPL_FUSE_ADAM=0"
    assert any(fused["m"])                                            # (the step did update)
