"""GPU: every regime of the 3x3 weight-gradient kernels (csrc/wgrad3x3.hip) against the fp64 oracle.

wgrad3b_kernel<CPR> (CPR 1 .. 11) and wgrad3b_pair_kernel<CA, CB> (seven pairs) each have three bodies chosen at run
time -- three bf16 pieces, two fp16 pieces (when the step left its maxima table), two pieces on a compacted sample list
(when some samples have an all-zero gradient image) -- and what is easiest to get wrong in them runs only when a
workgroup walks MORE THAN ONE stage: the double-buffered hand-off, and the carried-offset advance of `fetch` (the one
place a stage crosses a sample boundary; its constants change character with U against UPS = H / 2).  The parity tests
elsewhere reach several stages at CPR 2, 5 and 10 only.  Each case of tests/wgrad_cases.py is there for ONE regime: the
library's plan (cmlpl_debug_wgrad3_plan) is asserted first -- the kernels, the pair launch, the stage counts, U against
UPS -- then BaseNet2's forward and backward run and every live gradient (the two 3x3 weights and biases are what is under
test; the rest is free) must lie within 2e-6 of its tensor's largest element of the oracle in fp64 with the device's ReLU
decisions (audited: at most 4 flips), the bound and the rule of tests/test_gpu_shape_envelope.py.  The fp32 oracle's own
distance is printed next to the device's; no case needs the 4 x rule (docs/EXPERIMENTS.md, "Weight-gradient envelope").

The "stage" and "general" cases run again under CMLPL_WGRAD3_R / _PAIR / _B3 = 0 from tests/test_gpu_env_paths.py;
`under_switches` says what the plan must then be."""
import contextlib
import os

import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV, ModuleRegions, hip_relu_gates, relu_mask_audit
from tests.test_gpu_shape_envelope import BOUND, _inputs, _launch_counts, _module, _oracle
from tests.wgrad_cases import CASES, MAXCPR, PAIRS, check_plan, read_plan

pytestmark = pytest.mark.gpu
UNDER_TEST = ("grad conv1.weight", "grad conv1.bias", "grad conv2.weight", "grad conv2.bias")


@contextlib.contextmanager
def _switches(env):
    """CMLPL_* switches for the library calls inside; the environment and the library's table are restored"""
    from cmlpl_amd import _lib
    lib = _lib.load()
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    lib.cmlpl_debug_reload_switches()
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.cmlpl_debug_reload_switches()


def _two_piece(case):
    import ctypes as C
    from cmlpl_amd import _lib
    return _lib.load().cmlpl_debug_two_piece(C.byref(_lib.Shape(*case.shape)), 1, case.n)


def _run(case, zero=None, poison=None, label=""):
    """plan asserted, forward + backward, every live gradient against the fp64 oracle -> (device gradients, errors)
    zero: rows whose upstream gradients (dlog, dfe) are set to zero; poison: (row, value) put into x[row, 0, 0, 0] -- then
    only the finite / non-finite pattern and the finite elements of conv1's gradients are compared (returned, not asserted)"""
    shape, params, x, y, dm, dlog, dfe = _inputs(case)
    n = case.n
    if zero is not None:
        dlog[zero] = 0
        dfe[zero] = 0
    if poison is not None:
        x[poison[0], 0, 0, 0] = poison[1]
    plan = read_plan(case.shape, 1, n)
    print(f"[{case.id}{label}] {case.why}: {plan}")
    check_plan(case, plan)
    net = _module(shape, params, dropout=0.8)
    net.train()
    cnt = {}
    lo, fe = net(x.to(DEV), y.to(DEV), dropmask=dm.to(DEV))
    torch.cuda.synchronize()
    regions = ModuleRegions(net, lo, n)
    gates = hip_relu_gates(regions, shape, n)[0]
    with _launch_counts(cnt):
        ((lo * dlog.to(DEV)).sum() + (fe * dfe.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
    assert cnt["conv1_wgrad"] == 1 and cnt["conv1_wred"] == 1, cnt
    hip = dict(net.named_parameters())
    got = {"grad " + k: hip[k].grad.detach().cpu() for k in O.LIVE_KEYS}
    taps = {}
    ref = _oracle(params, x, y, dm, dlog, dfe, gates, torch.float64, taps)
    if poison is not None:
        return got, ref
    flips = relu_mask_audit(regions, [taps], shape, n)[0]
    assert sum(flips.values()) <= 4, flips
    ref32 = _oracle(params, x, y, dm, dlog, dfe, gates, torch.float32)

    def rel(a, b):
        return float((a.double() - b).abs().max() / b.abs().max())
    errs = {k: rel(got[k], ref[k]) for k in got}
    own = {k: rel(ref32[k], ref[k]) for k in got}
    print({k: f"{v:.2e} (fp32 oracle {own[k]:.2e})" for k, v in errs.items()}, "flips", flips)
    assert all(np.isfinite(v) for v in errs.values()) and max(errs.values()) < BOUND, errs
    return got, errs


TABLE = [c for c in CASES if c.tag in ("stage", "general")]


@pytest.mark.parametrize("case", TABLE, ids=[c.id for c in TABLE])
def test_weight_gradients_against_the_fp64_oracle_in_their_regime(case):
    _run(case)


FEW = [c for c in CASES if c.tag == "few"]


@pytest.mark.parametrize("rg", ("1", "2"))
@pytest.mark.parametrize("case", FEW, ids=[c.id for c in FEW])
def test_one_or_two_workgroups_walk_the_whole_batch(case, rg):
    """CMLPL_WGRAD3_RG: one or two workgroups per kernel row take every stage of every sample, two of them splitting in
    mid-sample -- held to the oracle, not to the default run"""
    with _switches({"CMLPL_WGRAD3_RG": rg}):
        _run(case, label=f" RG={rg}")


TWO = [c for c in CASES if c.tag == "stage" and c.two and c.pair]


@pytest.mark.parametrize("case", TWO, ids=[c.id for c in TWO])
def test_two_piece_body_against_the_fp64_oracle(case):
    """wgrad3b_body<CPR, true> in several stages at CPRs other than 5 and 10, behind the whole-sample kernels (12 x 12,
    14 x 14, 20 x 8) and behind the general ones (16 x 16 .. 20 x 20): the default run (already held to the oracle by the
    table) and the three-piece run of CMLPL_F16X2=0, each within the bound of fp64 by itself -- and not the same bits"""
    assert _two_piece(case) & 4
    g1, _ = _run(case)
    with _switches({"CMLPL_F16X2": "0"}):
        assert _two_piece(case) == 0
        g0, _ = _run(case, label=" F16X2=0")
    assert any(not torch.equal(g1[k], g0[k]) for k in UNDER_TEST[::2]), "the two-piece body did not run"


def _zero_rows(pattern, n):
    rows = torch.zeros(n, dtype=torch.bool)
    if pattern == "alternate":
        rows[1::2] = True
    elif pattern == "all-but-one":
        rows[:] = True
        rows[n // 3] = False
    else:
        rows[torch.randperm(n, generator=torch.Generator().manual_seed(5))[: n // 3]] = True
    return rows


SKIP_RUNS = [(c, p) for c in CASES for p in c.skip]


@pytest.mark.parametrize("case,pattern", SKIP_RUNS, ids=[f"{c.id}-{p}" for c, p in SKIP_RUNS])
def test_compacted_body_against_the_fp64_oracle(case, pattern):
    """wgrad3b_body<CPR, true, true>: samples whose upstream gradient rows are zero have an all-zero gradient image and are
    left out -- every other sample; all but one (most workgroups get an empty share: `ubeg` clipped to NU); a third of
    600 (both 512-wide loops of wgrad3b_run take a second trip).  The default run and the CMLPL_ZERO_SKIP=0 run are each
    within the bound of fp64; where they group the sums differently they are not the same bits (all-but-one may be: one
    sample's rows in one workgroup either way)."""
    zero = _zero_rows(pattern, case.n)
    assert read_plan(case.shape, 1, case.n).slist and _two_piece(case) & 4
    g1, _ = _run(case, zero=zero, label=" " + pattern)
    with _switches({"CMLPL_ZERO_SKIP": "0"}):
        assert not read_plan(case.shape, 1, case.n).slist
        g0, _ = _run(case, zero=zero, label=f" {pattern} ZERO_SKIP=0")
    if pattern != "all-but-one":
        assert any(not torch.equal(g1[k], g0[k]) for k in UNDER_TEST[::2]), "no sample was skipped"


def test_zero_gradient_sample_with_a_non_finite_activation_gives_the_oracles_nan():
    """0 x inf is NaN: a sample whose gradient image is zero must NOT be left out when its activations are not finite.  One
    input element of a zero-gradient sample is +inf (its corner pixel: conv0's output is +-inf there in all 64 channels),
    every other sample is ordinary.  conv1's weight gradient must be NaN exactly where the oracle's is (the taps that
    reach the corner) and within the bound elsewhere.  (The batch maximum of the activations is then not finite either, so
    wgrad3b_run takes the three-piece body, which walks every sample; the list build's own `>> 23 == 255` clause guards
    the same case should that order ever change.)"""
    case = next(c for c in CASES if c.poison)
    zero = _zero_rows("alternate", case.n)
    row = int(torch.nonzero(zero)[0])
    got, ref = _run(case, zero=zero, poison=(row, float("inf")), label=" poisoned")
    for k in ("grad conv1.weight", "grad conv1.bias"):
        bad = ~torch.isfinite(ref[k])
        print(k, "non-finite in the oracle:", int(bad.sum()), "of", bad.numel(), "on the device:", int((~torch.isfinite(got[k])).sum()))
        assert torch.equal(~torch.isfinite(got[k]), bad), k
        if k == "grad conv1.weight":
            assert bad.any() and not bad.all()
        fin = ~bad
        scale = ref[k][fin].abs().max()
        assert float((got[k].double()[fin] - ref[k][fin]).abs().max() / scale) < BOUND, k


def test_every_kernel_of_the_table_runs_in_several_stages():
    """the table itself, on THIS device: every CPR of wgrad3b_kernel and every instantiated pair kernel in at least one
    case whose workgroups run two stages or more (of both maps: the pairs)"""
    staged, pairs = set(), set()
    for case in CASES:
        plan = read_plan(case.shape, 1, case.n)
        staged.update(m.cpr for m in plan.maps if m.b3 and m.stages >= 2)
        if plan.pair and all(m.stages >= 2 for m in plan.maps):
            pairs.add(tuple(m.cpr for m in plan.maps))
    assert staged == set(range(1, MAXCPR + 1)) and pairs == set(PAIRS), (staged, pairs)
