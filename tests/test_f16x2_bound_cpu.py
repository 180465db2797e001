"""CPU: the per-element bound of the two-fp16-piece products (tests/f16x2_bound.py, derived in its docstring) against an
exact emulation of the scheme on the fp32 oracle's own operands, for every family of tests/f16x2_cases.py -- and the
proof that the bound can fail: on the wide-range inputs (channels falling off to 2^-28 of the sample's maximum, the
regime the absolute term exists for) a scale constant one binade off, a dropped second piece and flushed fp16
subnormals each break it.  The router's answer for every case is asked first (no device needed).
tests/test_gpu_f16x2_range.py holds the kernels to the same bound on the same inputs."""
import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests import f16x2_bound as B
from tests.f16x2_cases import CASES, FOUR_WAVE, assert_route, route

IDS = [c.id for c in CASES]


def _images(case, wide):
    shape = O.NetShape(*case.shape)
    params = O.closed_form_params(shape, 9)
    if wide:
        params = B.wide_range_params(params)
    x, y, dlog = B.inputs(shape, case.n, 77)
    im = B.oracle_images(params, x, y, dlog)
    lo, _ = O.basenet2_forward(params, x, y, None)
    assert torch.equal(lo, im["logits"])                       # the spelled-out forward IS the oracle's
    return params, im


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_router_answers_as_the_table_says(case):
    assert_route(case)


def test_four_wave_variant_appears_at_the_stated_row_count():
    fw = FOUR_WAVE
    at = route(fw["shape"], fw["nets"], fw["n"])
    below = route(fw["shape"], fw["nets"], fw["n"] - 1)
    assert at["fwd_ps"] == at["bwd_ps"] == fw["ps"] and (at["fwd"], at["bwd"], at["two_piece"]) == ("A", "A", 7)
    assert below["fwd_ps"] == below["bwd_ps"] == (8, 1, 1)


@pytest.mark.parametrize("wide", [False, True], ids=["unit", "wide-range"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_emulation_meets_the_bound_in_every_element(case, wide):
    params, im = _images(case, wide)
    w1, b1, w2, b2 = (params[k] for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"))
    H, W = case.shape[1:3]
    worst = {}
    # forward: conv1 on a0, conv2 on p1
    for name, a, w, b, gate in (("conv1 fwd", im["a0"], w1, b1, im["gate1"]), ("conv2 fwd", im["p1"], w2, b2, im["gate2"])):
        assert all(B.E_LO <= e <= B.E_HI for e in B.expos(a))
        worst[name] = B.worst(B.emulate_stage(a, w, b, gate), B.forward_stage(a, w, b, gate))
    # data gradient: conv1^T on dz1, conv2^T on dz2
    for name, dz, w in (("conv1 dgrad", im["dz1"], w1), ("conv2 dgrad", im["dz2"], w2)):
        worst[name] = B.worst(B.emulate_stage(dz, B.transposed(w), None), B.dgrad_stage(dz, w))
    # weight gradients: batch scales
    for name, a, dz in (("conv1 wgrad", im["a0"], im["dz1"]), ("conv2 wgrad", im["p1"], im["dz2"])):
        st = B.wgrad_stage(a, dz)
        assert B.wgrad_two_piece(st["ea"], st["eg"])
        worst[name] = B.worst(B.emulate_wgrad(a, dz), st)
    # the fp32 oracle's own figure beside it (against the plain c S: it has no scales)
    st = B.forward_stage(im["a0"], w1, b1, im["gate1"])
    worst["oracle fp32 conv1 fwd / plain"] = B.worst(im["p1"], st, "plain")
    print(f"[{case.id} {'wide' if wide else 'unit'}] err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for k, v in worst.items()), worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_range_case_is_not_vacuous(case):
    """from the oracle alone: the weights keep the range flag clear, every image maximum is inside the accepted exponents,
    and for at least a quarter of p1's elements the ABSOLUTE term u_s W_i is the larger part of the bound"""
    params, im = _images(case, True)
    for k in ("conv1.weight", "conv2.weight"):
        assert float(params[k].abs().max()) * 8192.0 <= 65000.0
    assert float(params["conv1.weight"].abs().max()) > 2.0                 # (weights "up to about 4")
    assert all(B.E_LO <= e <= B.E_HI for e in B.expos(im["a0"]))
    st = B.forward_stage(im["a0"], params["conv1.weight"], params["conv1.bias"], im["gate1"])
    live = st["S"] > 0
    share = float(((st["abs"] > st["plain"]) & live).sum()) / float(st["S"].numel())
    print(f"[{case.id}] elements whose absolute term exceeds 2^-18 S_i: {share:.3f} of p1")
    assert share >= 0.25, share
    # ... and the small channels are where they were put: 2^-k of the sample's maximum
    k = B.channel_k()
    mx = im["a0"].abs().amax(dim=(0, 2, 3))
    assert float(mx[k == 28].max()) < float(mx[k == 0].max()) * 2.0 ** -24


@pytest.mark.parametrize("wrong", ["scale_high", "no_h2", "flush"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wrong_emulations_break_the_bound_on_the_wide_range_case(case, wrong):
    """the proof that the GPU test can fail: each fault leaves the unit-scale comparisons against the tensor's largest
    element untouched (checked for the two subtle ones) and breaks the per-element bound"""
    params, im = _images(case, True)
    w1, b1 = params["conv1.weight"], params["conv1.bias"]
    st = B.forward_stage(im["a0"], w1, b1, im["gate1"])
    got = B.emulate_stage(im["a0"], w1, b1, im["gate1"], wrong=wrong)
    r = B.worst(got, st)
    vs_max = float((got - st["p"]).abs().max() / st["p"].abs().max())
    print(f"[{case.id}] {wrong}: err / bound {r:.3g}; against the largest element {vs_max:.3g}")
    assert r > 1.0, (wrong, r)
    if wrong == "flush":
        assert vs_max < 2e-6            # invisible to a comparison against the tensor's maximum
    # the weight gradient of the small channels breaks the same way
    stw = B.wgrad_stage(im["a0"], im["dz1"])
    assert B.worst(B.emulate_wgrad(im["a0"], im["dz1"], wrong=wrong), stw) > 1.0


def test_flushed_bound_is_the_wider_one_and_holds_for_the_flushing_emulation():
    """what the kernels would be held to if the hardware flushed fp16 subnormals (u = 2^(E - 28)): stated, and met by the
    flushing emulation -- the fall-back the GPU tests document, not use, unless the device does flush"""
    case = CASES[0]
    params, im = _images(case, True)
    w1, b1 = params["conv1.weight"], params["conv1.bias"]
    st = B.forward_stage(im["a0"], w1, b1, im["gate1"], flushed=True)
    assert B.worst(B.emulate_stage(im["a0"], w1, b1, im["gate1"], wrong="flush"), st) <= 1.0
    assert (st["bound"] >= B.forward_stage(im["a0"], w1, b1, im["gate1"])["bound"]).all()
