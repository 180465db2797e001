"""GPU: the loop structure of the gradient fold (csrc/conv0.hip: conv0_fold, partial_reduce_block, reduce_adam_block) at
the smallest shapes where it can go wrong.

The number of partial rows G of conv0's fold is min(rows per network, 256) on the general backward route (ROUTE_C) and
the rows per network, uncapped, on the per-sample routes.  conv0's blocks take four groups of 32 rows per round trip,
the unfused fold of a 3x3 tensor two.  The cases:
  w8c5   8 x 8 windows, C = 5: conv0's partial has 8 rows of 64 + 64 bias sums = 576 elements = 4.5 blocks of 128, so
         the bias tail shares a block with the body and the block's upper half lies past the partial.  This shape takes
         the GENERAL route at every batch: G is one below, at and one above every multiple of 32 up to 160 (four
         groups in flight plus one), and 260 rows give G = 256, the cap;
  w12c5  12 x 12, C = 5, a PER-SAMPLE route: 129 rows, and 260 rows with G = 260 -- a third trip round conv0's loop;
  w8c103 C = 103 (104 partial rows: the padded row 103 is folded but belongs to no parameter), per-sample, G = 65.
The route of every case is asserted (cmlpl_debug_route), so that the G named here is the G that ran.

Each case runs ONE training step (backward + update) through the C ABI twice from the same state -- the default path,
asserted by its launch counts to be the fused fold + Adam launch, and CMLPL_FUSE_ADAM=0 (reduce_gemm_kernel +
adam_kernel, asserted likewise), the switches re-read in process -- and asserts
  1. gradients, parameters, m, v and the packed block are byte-equal between the two paths;
  2. all ten gradient tensors agree with the fp64 oracle at the bound tests/test_gpu_step.py holds gradients to.
Both paths call the same conv0_fold, so (1) holds the two block structures around it to each other, not the summation
association: what checks the association is (2) and, outside this suite, the byte comparison of the benchmark's outputs
with those of the commit before the change.
The oracle alone is checked (without a GPU) to give finite, non-zero conv0 gradients at these shapes, so that (2) is
not vacuous.
"""
import ctypes as C
import os

import pytest
import torch

from oracle import cmlpl_oracle as O

DEV = "cuda:0"
ROUTE_C = 2
SHAPES = {"w8c5": O.NetShape(5, 8, 8, 5, 9), "w12c5": O.NetShape(5, 12, 12, 5, 9), "w8c103": O.NetShape(103, 8, 8, 103, 9)}
ROWS = (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 260)
# (shape, rows per network, conv0's backward on the general route?)
CASES = [("w8c5", n, True) for n in ROWS] + [("w12c5", 129, False), ("w12c5", 260, False), ("w8c103", 65, False)]
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
def test_the_oracle_alone_gives_finite_nonzero_conv0_gradients(name):
    shape = SHAPES[name]
    bt, btu = _split(33)
    p0, p1 = _state(name)
    hp = O.HyperParams()
    st = O.StepState.create(shape, p0, p1, bt, hp)
    b = O.synthetic_batch(shape, bt, btu, 77)
    ref = O.train_step(st, b["XPl"], b["Xl"], b["Y"], b["XPu"], b["Xu"], b["noise"], b["dropmask"], 1, 0, hp)
    for net in range(2):
        for k in ("conv0.weight", "conv0.bias"):
            g = ref["grads"][net][k]
            assert torch.isfinite(g).all(), (net, k)
            nz = int((g != 0).sum())
            print(f"[{name}] oracle grad[{net}] {k}: max|g|={float(g.abs().max()):.3e}, {nz}/{g.numel()} non-zero")
            assert nz > g.numel() // 2 and float(g.abs().max()) > 1e-6, (net, k, nz)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,general", CASES, ids=[f"{a}-{n}" for a, n, _ in CASES])
def test_both_folds_are_byte_equal_and_meet_the_oracle(name, n, general):
    from cmlpl_amd import _lib
    from tests.gpu_util import hip_relu_gates, report
    shape = SHAPES[name]
    route = (C.c_int * 40)()
    _lib.check("cmlpl_debug_route", _lib.load().cmlpl_debug_route(
        C.byref(_lib.Shape(shape.C, shape.H, shape.W, shape.bands, shape.K)), 2, n, route))
    assert (route[1] == ROUTE_C) == general, f"{name} n={n}: backward route {route[1]}"
    bt, btu = _split(n)
    hp = O.HyperParams()
    b = O.synthetic_batch(shape, bt, btu, 77)
    eng, fused, c_fused = _step(name, n, None, b)
    assert c_fused["conv1_wred"] == 1 and c_fused["adam"] == 0, c_fused      # the fused fold + Adam launch
    # (2) the oracle with the device's ReLU decisions, as tests/test_gpu_step.py compares gradients
    st = O.StepState.create(shape, *_state(name), bt, hp)
    ref = O.train_step(st, b["XPl"], b["Xl"], b["Y"], b["XPu"], b["Xu"], b["noise"], b["dropmask"], 1, 0, hp,
                       relu_gates=hip_relu_gates(eng, shape, n))
    assert len(O.LIVE_KEYS) == 10
    for net in range(2):
        for k in O.LIVE_KEYS:
            gr = ref["grads"][net][k]
            mx = max(float(gr.abs().max()), 1e-4)
            report(f"[{name} n={n}] grad[{net}] {k}", eng.grad(net, k), gr, 5e-4, 5e-5 * mx)
    del eng
    # (1) the two launches it replaces
    _, two, c_two = _step(name, n, "0", b)
    assert c_two["conv1_wred"] == 1 and c_two["adam"] >= 1, c_two
    for f in FIELDS:
        assert fused[f] == two[f], f"{name} n={n}: `{f}` differs between the fused fold and CMLPL_FUSE_ADAM=0"
    assert any(fused["m"])                                            # (the step did update)
