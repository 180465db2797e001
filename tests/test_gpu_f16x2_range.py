"""GPU: the two-fp16-piece loops at the EDGES of the ranges they accept and element by element
against fp64 -- what tests/test_gpu_f16x2.py (fall-backs 25 binades from an edge, errors against the tensor's largest
element) cannot see: a wrong exponent constant, a scale word shared between two samples, a second piece or an fp16
subnormal that is flushed.

Every reference is an fp64 re-computation from the DEVICE'S OWN operands and ReLU decisions (tests/f16x2_bound.py: the
saved regions a0 / p1 / dp1 / dp2 / m1 / m2), so only the loop under test differs, and every bound is the derived one of
that module (checked on the CPU, with three wrong emulations that break it, in tests/test_f16x2_bound_cpu.py).  A sample
/ batch outside the ranges must equal the CMLPL_F16X2=0 run byte for byte; one inside must differ from it (the loop ran)
and meet the bound in every element.  To make "byte for byte" a statement about the loop alone, the stage IN FRONT of the
one under test is given zero weights where its own loop choice could change the operand (then its output is the residual,
exactly, on either loop); the tests assert that the operands of the two runs are the same bytes.

The families and what the router launches for them: tests/f16x2_cases.py (asserted before anything runs)."""
import contextlib
import os

import pytest
import torch

from oracle import cmlpl_oracle as O
from tests import f16x2_bound as B
from tests.f16x2_cases import CASES, EDGE_EXPONENTS, FOUR_WAVE, WGRAD_CORNERS, assert_route, route
from tests.gpu_util import DEV, ModuleRegions, hip_relu_gates

pytestmark = pytest.mark.gpu
IDS = [c.id for c in CASES]
GENERAL = [c for c in CASES if c.conv2_two_piece]


@contextlib.contextmanager
def switches(**env):
    """CMLPL_* switches for the library calls inside; re-read in process, the environment as before afterwards"""
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


def run(case, params, x, y, dlog=None, f16x2="1"):
    """one forward (and backward) of a BaseNet2 module under CMLPL_F16X2 -> the saved regions as fp32 [n][pixels][64] CPU
    tensors, the ReLU masks (bytes and gates), the three convolutions' weight gradients and the weight-range flag word"""
    from cmlpl_amd import _lib
    from cmlpl_amd.models import BaseNet2
    shape, n = O.NetShape(*case.shape), x.shape[0]
    H, W = shape.H, shape.W
    with switches(CMLPL_F16X2=f16x2):
        net = BaseNet2(num_features=shape.bands, dropout=0.0, num_classes=shape.K, in_channels=shape.C,
                       window=(H, W)).to(DEV)
        net.load_state_dict(params)
        net.train()
        lo, _ = net(x.to(DEV), y.to(DEV))
        reg = ModuleRegions(net, lo, n)
        if dlog is not None:
            (lo * dlog.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        out = {"n": n}
        sizes = {"a0": H * W, "p1": (H // 2) * (W // 2), "p2": (H // 4) * (W // 4)}
        if dlog is not None:
            sizes.update({"dp1": sizes["p1"], "dp2": sizes["p2"]})
            if case.da0_in_hbm:
                sizes["da0"] = H * W
        for name, px in sizes.items():
            out[name] = reg.debug_region(name).view(-1)[: n * px * 64].view(n, px, 64).cpu().clone()
        for name in ("m1", "m2"):
            out[name] = reg.debug_region(name, torch.uint8).cpu().clone()
        out["gate"] = hip_relu_gates(reg, shape, n)[0]
        if dlog is not None:
            named = dict(net.named_parameters())
            for k in ("conv0.weight", "conv1.weight", "conv2.weight"):
                out["d" + k] = named[k].grad.detach().cpu().clone()
        pt = int(_lib.layout(net._cshape).packed_total)
        out["flag"] = int(net._cache[2][pt - 16: pt - 15].view(torch.int32).item())      # the weight-range flag word
    return out


def img(r, name, h, w):
    """region `name` of a run as fp64 [n, 64, h, w]"""
    return r[name].double().permute(0, 2, 1).reshape(r["n"], 64, h, w)


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def params_of(case, seed=9):
    return O.closed_form_params(O.NetShape(*case.shape), seed)


# the samples of an edge batch: the exponent field the image's maximum is placed at; "den": a denormal maximum; "zero": an
# all-zero image; "nan": one NaN in an otherwise ordinary image
FWD_SAMPLES = [("e", e) for e in EDGE_EXPONENTS] + [("den", -1), ("zero", None), ("nan", 127)]
BWD_SAMPLES = [("e", e) for e in EDGE_EXPONENTS] + [("zero", None)]


def scaled(t, unit_exps, samples):
    """t's rows scaled by powers of two (exact) so that images whose maxima had the exponent fields `unit_exps` land on
    the samples' targets; "zero" rows are zeroed"""
    t = t.clone()
    for s, (kind, e) in enumerate(samples):
        if kind == "zero":
            t[s] = 0
        else:
            assert 0 < unit_exps[s] < 255
            q = e - unit_exps[s]
            t[s] = t[s] * B.pow2(q // 2) * B.pow2(q - q // 2)       # (two factors, each an ordinary fp32 number)
    return t


def check_samples(tag, case, samples, image, got1, got0, st, nan_must_reach=True):
    """the assertions of an edge batch.  image [n,64,h,w]: the operand images of the loop under test (the device's, both
    runs the same bytes: asserted by the caller); got1 / got0 [n, ...]: the loop's output per sample under CMLPL_F16X2 = 1 /
    0; st: the fp64 stage of the CMLPL_F16X2 = 1 run.  `nan_must_reach`: the NaN is in the image under test (conv2's image
    is behind conv1's ReLU, which may drop it: then the sample is one more ordinary one at exponent 127)."""
    exps = B.expos(image)
    worst = {}
    for s, (kind, e) in enumerate(samples):
        if kind == "zero":
            assert not bool((image[s] != 0).any()), (tag, s)
            assert bool((got1[s] == 0).all()), (tag, s, "a zero image (and no bias) must give exact zeros")
            continue
        if kind == "den":
            assert exps[s] == 0, (tag, s, exps[s])                  # (a device that flushes it leaves a zero image: same verdict)
        elif kind == "nan" and (nan_must_reach or exps[s] == 255):
            assert exps[s] == 255 and bool(torch.isnan(image[s]).any()), (tag, s, exps[s])
        else:
            assert exps[s] == e, (tag, s, exps[s], e)               # from the device's region, not from the plan
        if B.E_LO <= exps[s] <= B.E_HI:
            assert not same_bytes(got1[s], got0[s]), (tag, s, exps[s], "the two-piece loop did not run")
            err = (got1[s].double() - st["p"][s]).abs()
            r = torch.where(err == 0, B.ZERO, err / st["bound"][s])
            worst[exps[s]] = max(worst.get(exps[s], 0.0), float(torch.nan_to_num(r, nan=float("inf")).max()))
        else:
            assert same_bytes(got1[s], got0[s]), (tag, s, exps[s], "not the three-piece loop's bytes")
    print(f"[{case.id}] {tag}: exponents {exps}; largest err / bound per in-range exponent "
          + ", ".join(f"{e}: {v:.3f}" for e, v in sorted(worst.items())))
    assert set(worst) == {40, 41, 127, 199, 200}, worst
    assert max(worst.values()) <= 1.0, (tag, worst)
    return worst


# ------------------------------------------------------------------------------------------------ 3a: forward edges
def forward_edges(case, stage):
    assert_route(case)
    shape = O.NetShape(*case.shape)
    H, W = shape.H, shape.W
    n = len(FWD_SAMPLES)
    params = B.no_conv_bias(params_of(case))
    if stage == 2:
        params["conv1.weight"] = torch.zeros_like(params["conv1.weight"])       # p1 = pool(relu(a0)) exactly, on either loop
    x, y, _ = B.inputs(shape, n, 31)
    name, h, w = ("a0", H, W) if stage == 1 else ("p1", H // 2, W // 2)
    out, oh, ow = ("p1", H // 2, W // 2) if stage == 1 else ("p2", H // 4, W // 4)
    wk, bk, gk = f"conv{stage}.weight", f"conv{stage}.bias", f"z{stage}"
    unit = B.expos(img(run(case, params, x, y), name, h, w))
    xs = scaled(x, unit, FWD_SAMPLES)
    xs[[k for k, _ in FWD_SAMPLES].index("nan"), 0, H // 2 - 1, W // 2 - 1] = float("nan")
    r1, r0 = run(case, params, xs, y, f16x2="1"), run(case, params, xs, y, f16x2="0")
    assert r1["flag"] == 0 and r0["flag"] == 0
    assert same_bytes(r1[name], r0[name]), "the operand images of the two runs differ"
    image = img(r1, name, h, w)
    clean = torch.nan_to_num(image, nan=0.0)                       # (the NaN sample is never held to a bound)
    st = B.forward_stage(clean, params[wk], params[bk], r1["gate"][gk])
    res = check_samples(f"conv{stage} forward", case, FWD_SAMPLES, image, img(r1, out, oh, ow), img(r0, out, oh, ow), st,
                        nan_must_reach=(stage == 1))
    # the zero sample with the stage's bias in place: the bias pattern, exactly (relu, and a mean of four equal numbers)
    pb = dict(params)
    pb[bk] = params_of(case)[bk]
    rb = run(case, pb, xs, y)
    zs = [k for k, _ in FWD_SAMPLES].index("zero")
    want = torch.relu(pb[bk]).double().view(64, 1, 1).expand(64, oh, ow)
    assert bool((img(rb, out, oh, ow)[zs] == want).all()), "zero image: not the bias pattern"
    return res


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv1_forward_decision_edges_in_one_batch(case):
    """ONE batch whose a0 maxima sit at the exponent fields 39 / 40 / 41 / 127 / 199 / 200 / 201 (conv0 is a 1x1 convolution
    without ReLU: with its bias zero a sample's input scaled by 2^q scales its a0 exactly), plus a denormal-maximum, an
    all-zero and a one-NaN sample: a scale belongs to its sample alone."""
    forward_edges(case, 1)


@pytest.mark.parametrize("case", GENERAL, ids=[c.id for c in GENERAL])
def test_conv2_forward_decision_edges_in_one_batch(case):
    """the same for conv2's own launch (general path: p1 -> p2), the exponents placed on p1's maxima"""
    forward_edges(case, 2)


# ---------------------------------------------------------------------------------------- 3a: data-gradient edges
def probe_positions(H, W):
    """corners, edge midpoints, (on an odd map these include the last row and column the pool drops), interior"""
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, W // 2), (H // 2, W - 1),
           (H // 2, W // 2), (1, 1), (H - 2, W - 2)]
    return list(dict.fromkeys(pos))


def backward_edges(case, stage):
    assert_route(case)
    shape = O.NetShape(*case.shape)
    H, W, C = shape.H, shape.W, shape.C
    n = len(BWD_SAMPLES)
    params = params_of(case)
    # The two runs' forwards differ by rounding (two pieces or three), and a ReLU decision within that rounding of zero
    # would change a gradient image for a reason that is not the loop under test.  The stage whose masks shape the image
    # gets a bias of +-8 per channel (two channels in three open): every pre-activation is far from zero, the decisions
    # are the bias's sign in both runs (asserted below).  The gradient image is as general as before inside the open
    # channels and zero in the others.
    pm8 = torch.where(torch.arange(64) % 3 == 0, -8.0, 8.0)
    params[f"conv{stage}.bias"] = pm8
    if stage == 1:
        params["conv2.weight"] = torch.zeros_like(params["conv2.weight"])       # dp1 = dz2 exactly, on either loop
        params["conv2.bias"] = torch.zeros_like(params["conv2.bias"])           # ... and conv2's decisions are p1 > 0
    _, y, dlog = B.inputs(shape, n, 57)
    fused = stage == 1 and not case.da0_in_hbm
    if fused:
        # da0 stays on chip: read it through conv0's weight gradient.  Every input channel is a one-hot image (one pixel
        # set to 1.0 in one sample), so conv0.weight.grad[co][c] IS da0[s(c)][co][pixel(c)]: products with 1.0 and sums
        # with zeros are exact on the three-piece path.
        probes = [(s, h, w) for s in range(n) for (h, w) in probe_positions(H, W)]
        k = 0
        while len(probes) % C:                                      # fill the last pass: more interior pixels
            probes.append((k % n, 2 + k % (H - 4), 2 + (3 * k) % (W - 4)))
            k += 1
        passes = [probes[i: i + C] for i in range(0, len(probes), C)]
    else:
        passes = [None]
    dpn, mh, mw = ("dp1", H // 2, W // 2) if stage == 1 else ("dp2", H // 4, W // 4)
    ih, iw = (H, W) if stage == 1 else (H // 2, W // 2)
    wk, gk = f"conv{stage}.weight", f"z{stage}"
    differs, worst, seen = [False] * n, {}, set()
    for pr in passes:
        if fused:
            x = torch.zeros(n, C, H, W)
            for c, (s, h, w) in enumerate(pr):
                x[s, c, h, w] = 1.0
        else:
            x = B.inputs(shape, n, 58)[0]
        ru = run(case, params, x, y, dlog)
        unit = B.expos(B.grad_image(img(ru, dpn, mh, mw), ru["gate"][gk], ih, iw))
        dls = scaled(dlog, unit, BWD_SAMPLES)
        r1, r0 = run(case, params, x, y, dls, "1"), run(case, params, x, y, dls, "0")
        assert r1["flag"] == 0
        for m in (("m1", "m2") if stage == 1 else ("m2",)):           # the decisions that shape this gradient image
            assert torch.equal(r1[m], r0[m]), (m, "a ReLU decision flipped between the runs")
        assert same_bytes(r1[dpn], r0[dpn]), "the gradient images of the two runs differ"
        dz = B.grad_image(img(r1, dpn, mh, mw), r1["gate"][gk], ih, iw)
        st = B.dgrad_stage(dz, params[wk])
        exps = B.expos(dz)
        if fused:
            g1, g0 = r1["dconv0.weight"].view(64, C), r0["dconv0.weight"].view(64, C)
            cols = lambda s: [c for c, p in enumerate(pr) if p[0] == s]
            pick = lambda t, s: torch.stack([t[s, :, pr[c][1], pr[c][2]] for c in cols(s)], 1) if cols(s) else torch.zeros(64, 0, dtype=t.dtype)
            outs = [(g1[:, cols(s)], g0[:, cols(s)], pick(st["p"], s), pick(st["bound"], s)) for s in range(n)]
        else:
            on, oh, ow = ("da0", H, W) if stage == 1 else ("dp1", H // 2, W // 2)     # (conv2's data gradient writes dp1)
            o1, o0 = img(r1, on, oh, ow), img(r0, on, oh, ow)
            outs = [(o1[s], o0[s], st["p"][s], st["bound"][s]) for s in range(n)]
        for s, (kind, e) in enumerate(BWD_SAMPLES):
            a1, a0_, ref, bound = outs[s]
            if a1.numel() == 0:
                continue
            seen.add(s)
            if kind == "zero":
                assert not bool((dz[s] != 0).any())
                assert bool((a1 == 0).all()), (s, "a zero gradient image must give exact zeros")
                continue
            assert exps[s] == e, (s, exps[s], e)
            if B.E_LO <= e <= B.E_HI:
                differs[s] = differs[s] or not same_bytes(a1.float(), a0_.float())
                err = (a1.double() - ref).abs()
                r = torch.where(err == 0, B.ZERO, err / bound)
                worst[e] = max(worst.get(e, 0.0), float(torch.nan_to_num(r, nan=float("inf")).max()))
            else:
                assert same_bytes(a1.float(), a0_.float()), (s, e, "not the three-piece loop's bytes")
    assert seen == set(range(n))
    for s, (kind, e) in enumerate(BWD_SAMPLES):
        if kind == "e" and B.E_LO <= e <= B.E_HI:
            assert differs[s], (s, e, "the two-piece loop did not run")
    print(f"[{case.id}] conv{stage} data gradient ({'through dW0 probes, %d passes' % len(passes) if fused else 'region'}): "
          "largest err / bound per in-range exponent " + ", ".join(f"{e}: {v:.3f}" for e, v in sorted(worst.items())))
    assert set(worst) == {40, 41, 127, 199, 200} and max(worst.values()) <= 1.0, worst
    return worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv1_data_gradient_decision_edges_in_one_batch(case):
    """unit-scale forward; the rows of the upstream gradient scaled by powers of two so that conv1's gradient images (the
    masked, up-sampled dp1) sit at the edge exponents, one row with no gradient at all (the zero-image skip: da0 exactly
    zero).  dp1 -> da0; where da0 stays on chip it is read through conv0's weight gradient of one-hot input channels."""
    backward_edges(case, 1)


@pytest.mark.parametrize("case", GENERAL, ids=[c.id for c in GENERAL])
def test_conv2_data_gradient_decision_edges_in_one_batch(case):
    """the same for conv2's own launch (general path): dp2 -> dp1"""
    backward_edges(case, 2)


# --------------------------------------------------------------------------- 3b: a wide range inside one sample
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_range_inside_one_sample_on_the_two_piece_path(case):
    """conv0's output channels fall off by 2^-k, k = 0 / 12 / 16 / 17 / 18 / 20 / 24 / 28, NOT undone in conv1, and a block of
    conv1's output channels reads the small channels only (tests/f16x2_bound.py: wide_range_params; the flag stays
    clear): every element of p1 meets the derived bound, the run is not the three-piece run, the three-piece run of the
    same inputs meets the plain 2^-18 S_i with no absolute term (the inputs are fair: the difference between the two bounds
    is the scheme's documented trade), and conv1's weight gradient -- whose elements of the small input channels have no
    large term to hide behind -- meets the weight-gradient bound in every element."""
    assert_route(case)
    shape = O.NetShape(*case.shape)
    H, W = shape.H, shape.W
    params = B.wide_range_params(params_of(case))
    x, y, dlog = B.inputs(shape, case.n, 77)
    r1, r0 = run(case, params, x, y, dlog, "1"), run(case, params, x, y, dlog, "0")
    assert r1["flag"] == 0 and r0["flag"] == 0
    a0 = img(r1, "a0", H, W)
    assert same_bytes(r1["a0"], r0["a0"]) and all(B.E_LO <= e <= B.E_HI for e in B.expos(a0))
    w1, b1 = params["conv1.weight"], params["conv1.bias"]
    k = B.channel_k()
    groups = sorted(set(k.tolist()))
    # forward
    st1 = B.forward_stage(a0, w1, b1, r1["gate"]["z1"])
    st0 = B.forward_stage(a0, w1, b1, r0["gate"]["z1"])
    p1_1, p1_0 = img(r1, "p1", H // 2, W // 2), img(r0, "p1", H // 2, W // 2)
    assert not same_bytes(r1["p1"], r0["p1"]), "the two-piece loop did not run"
    f_two, f_three = B.worst(p1_1, st1), B.worst(p1_0, st0, "plain")
    per_k = {kk: B.worst(p1_1[:, k == kk], {"p": st1["p"][:, k == kk], "bound": st1["bound"][:, k == kk]}) for kk in groups}
    binding = float(((st1["abs"] > st1["plain"]) & (st1["S"] > 0)).sum()) / st1["S"].numel()
    print(f"[{case.id}] wide range, p1: err / bound {f_two:.3f} (per k of the output channel: "
          + ", ".join(f"{kk}: {v:.3f}" for kk, v in per_k.items()) + f"); absolute term binding for {binding:.2f} of the elements; "
          f"three-piece run against the plain 2^-18 S_i: {f_three:.3f}; two-piece run against the plain bound: "
          f"{B.worst(p1_1, st1, 'plain'):.3f}")
    assert binding >= 0.25
    assert f_two <= 1.0, f_two
    assert f_three <= 1.0, f_three
    # weight gradients (conv1's: operands a0 and the masked up-sampled dp1; conv2's printed beside it)
    dz1 = B.grad_image(img(r1, "dp1", H // 2, W // 2), r1["gate"]["z1"], H, W)
    sw = B.wgrad_stage(a0, dz1)
    assert B.wgrad_two_piece(sw["ea"], sw["eg"])
    dw1 = r1["dconv1.weight"].double()
    assert not same_bytes(r1["dconv1.weight"], r0["dconv1.weight"])
    w_all = B.worst(dw1, sw)
    per_ki = {kk: B.worst(dw1[:, k == kk], {"p": sw["p"][:, k == kk], "bound": sw["bound"][:, k == kk]}) for kk in groups}
    dz2 = B.grad_image(img(r1, "dp2", H // 4, W // 4), r1["gate"]["z2"], H // 2, W // 2)
    sw2 = B.wgrad_stage(p1_1, dz2)
    w2_all = B.worst(r1["dconv2.weight"].double(), sw2)                     # (p1 is as wide as a0 here)
    print(f"[{case.id}] wide range, dW1: err / bound {w_all:.3f} (per k of the input channel: "
          + ", ".join(f"{kk}: {v:.3f}" for kk, v in per_ki.items()) + f"); dW2: {w2_all:.3f}")
    assert w_all <= 1.0, (w_all, per_ki)
    assert w2_all <= 1.0, w2_all


# ------------------------------------------------------------------------------- 3c: weight-gradient decision edges
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weight_gradient_decision_edges(case):
    """Whole small batches with the BATCH exponents (ea, eg) of conv1's, then of conv2's, operands at the corners of the
    rule -- 40 <= ea, eg <= 200 and ea + eg >= 160 -- read from the device's regions.  Both 3x3 convolutions have zero
    weights and biases here: a weight gradient does not depend on the weights' values, and then every operand (a0, p1 =
    pool(relu(a0)), the masks, dp1 = dz2) is the same bytes under either setting of the switch, so that a three-piece
    corner must equal the CMLPL_F16X2=0 run byte for byte; a two-piece corner differs from it and meets the bound in every
    element.  Last, one batch in which a single sample's activations and another's gradient are 2^30 above the rest: the
    batch scales are set by one sample each, and every element is held."""
    assert_route(case)
    shape = O.NetShape(*case.shape)
    H, W = shape.H, shape.W
    n = case.n
    params = B.no_conv_bias(params_of(case))
    for key in ("conv1.weight", "conv2.weight"):
        params[key] = torch.zeros_like(params[key])
    x, y, dlog = B.inputs(shape, n, 91)

    def operands(r):
        a0, p1 = img(r, "a0", H, W), img(r, "p1", H // 2, W // 2)
        dz1 = B.grad_image(img(r, "dp1", H // 2, W // 2), r["gate"]["z1"], H, W)
        dz2 = B.grad_image(img(r, "dp2", H // 4, W // 4), r["gate"]["z2"], H // 2, W // 2)
        return {1: (a0, dz1), 2: (p1, dz2)}

    def batch(xs, dls, tag, target=None, corner=None):
        r1, r0 = run(case, params, xs, y, dls, "1"), run(case, params, xs, y, dls, "0")
        assert r1["flag"] == 0
        for name in ("a0", "p1", "dp1", "dp2", "m1", "m2"):
            same = torch.equal(r1[name], r0[name]) if name[0] == "m" else same_bytes(r1[name], r0[name])
            assert same, (tag, name, "operands differ between the runs")
        line = []
        for g, (a, dz) in operands(r1).items():
            ea, eg = B.expo(a), B.expo(dz)
            if g == target:
                assert (ea, eg) == corner, (tag, g, (ea, eg), corner)       # from the device's regions
            d1, d0 = r1[f"dconv{g}.weight"], r0[f"dconv{g}.weight"]
            if B.wgrad_two_piece(ea, eg):
                assert not same_bytes(d1, d0), (tag, g, ea, eg, "the two-piece planes were not taken")
                st = B.wgrad_stage(a, dz)
                assert float(st["p"].abs().max()) > 2.0 ** -100           # (results that are normal fp32 numbers)
                ratio = B.worst(d1.double(), st)
                line.append(f"dW{g} ({ea},{eg}) two-piece {ratio:.3f}")
                assert ratio <= 1.0, (tag, g, ea, eg, ratio)
            else:
                assert same_bytes(d1, d0), (tag, g, ea, eg, "not the three-piece planes' bytes")
                line.append(f"dW{g} ({ea},{eg}) three-piece, same bytes")
        print(f"[{case.id}] {tag}: " + "; ".join(line))

    unit = {g: (B.expo(a), B.expo(dz)) for g, (a, dz) in operands(run(case, params, x, y, dlog)).items()}
    two = B.pow2
    for target in (1, 2):
        for corner in WGRAD_CORNERS:
            qa, qg = corner[0] - unit[target][0], corner[1] - unit[target][1]
            batch(x * two(qa), dlog * two(qg), f"conv{target}'s operands at {corner}", target, corner)
    xs, dls = x.clone(), dlog.clone()
    xs[0] *= 2.0 ** 30
    dls[1] *= 2.0 ** 30
    batch(xs, dls, "one sample 2^30 above the rest in each operand")


@pytest.mark.parametrize("case", GENERAL, ids=[c.id for c in GENERAL])
def test_conv2_weight_gradient_takes_its_scale_from_p1_not_from_p2(case):
    """Regression (found by test_weight_gradient_decision_edges on the general path): conv2's own forward launch wrote the
    maximum of ITS pooled map, p2, over the p1 maximum the weight gradient of conv2 scales its activations by.  Here conv2
    is -(1 - 2^-6) times the identity, so that z2 = 2^-6 p1 and p2 lies six binades below p1: a scale taken from p2 puts p1
    at 2^20 in fp16 pieces.  dW2 (which does not depend on conv2's values) must meet the weight-gradient bound in every
    element on its own operands."""
    assert_route(case)
    shape = O.NetShape(*case.shape)
    H, W = shape.H, shape.W
    params = B.no_conv_bias(params_of(case))
    w2 = torch.zeros_like(params["conv2.weight"])
    w2[torch.arange(64), torch.arange(64), 1, 1] = -(1.0 - 2.0 ** -6)
    params["conv2.weight"] = w2
    x, y, dlog = B.inputs(shape, case.n, 93)
    r1 = run(case, params, x, y, dlog, "1")
    p1, p2 = img(r1, "p1", H // 2, W // 2), img(r1, "p2", H // 4, W // 4)
    assert r1["flag"] == 0 and B.expo(p2) <= B.expo(p1) - 5, (B.expo(p1), B.expo(p2))
    dz2 = B.grad_image(img(r1, "dp2", H // 4, W // 4), r1["gate"]["z2"], H // 2, W // 2)
    st = B.wgrad_stage(p1, dz2)
    assert B.wgrad_two_piece(st["ea"], st["eg"])
    ratio = B.worst(r1["dconv2.weight"].double(), st)
    print(f"[{case.id}] p1 at exponent {B.expo(p1)}, p2 at {B.expo(p2)}: dW2 err / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


# ------------------------------------------------------------------------ the four-wave, four-tile per-sample kernels
def test_four_wave_kernels_equal_the_eight_wave_ones_on_a_mixed_range_batch():
    """(103, 11, 11) with two networks takes the four-wave, two-tiles-per-wave kernels from 129 rows per network on (asked of
    the router).  One TrainEngine step there on a batch whose rows are scaled over the whole exponent range -- in-range,
    out-of-range and all-zero images side by side -- against the same step on the eight-wave kernels (CMLPL_KS8=1):
    DESIGN.md states the two are bit-identical; the bytes of logits and gradients are compared."""
    from cmlpl_amd import HyperParams, NetShape, TrainEngine
    fw = FOUR_WAVE
    at, below = route(fw["shape"], fw["nets"], fw["n"]), route(fw["shape"], fw["nets"], fw["n"] - 1)
    assert at["fwd_ps"] == at["bwd_ps"] == fw["ps"] and below["fwd_ps"] == below["bwd_ps"] == (8, 1, 1)
    shape = O.NetShape(*fw["shape"])
    bt, btu = 64, fw["n"] - 64
    params = B.no_conv_bias(O.closed_form_params(shape, 9), keys=("conv0.bias",))
    b = O.synthetic_batch(shape, bt, btu, 41)
    qs = [-95, -89, -88, -87, -86, -40, 0, 40, 70, 71, 72, 73, 74, 80, None]          # None: an all-zero window
    def spread(t):
        t = t.clone()
        for s in range(t.shape[0]):
            q = qs[s % len(qs)]
            t[s] = 0 if q is None else t[s] * B.pow2(q)
        return t
    XPl, XPu = spread(b["XPl"]), spread(b["XPu"])

    def step(env):
        with switches(**env):
            eng = TrainEngine(NetShape(*fw["shape"]), bt, btu, HyperParams(noise=0.0), device=DEV, seed=3)
            for net in range(2):
                eng.load_state_dict(net, params)
            d = lambda t: t.to(DEV)
            eng.step(d(XPl), d(b["Xl"]), d(b["Y"]), d(XPu), d(b["Xu"]), 1, 0, apply_update=False)
            torch.cuda.synchronize()
            a0 = eng.debug_region("a0").view(2, fw["n"], shape.H * shape.W, 64)[0].cpu().clone()
            return eng.logits.clone().cpu(), eng.grads.clone().cpu(), a0

    lo4, g4, a0 = step({})
    lo8, g8, _ = step({"CMLPL_KS8": "1"})
    exps = B.expos(a0)
    inside = sum(B.E_LO <= e <= B.E_HI for e in exps)
    print(f"four waves against eight: {inside} of {len(exps)} images inside the two-piece range, exponents {sorted(set(exps))}")
    assert inside >= 30 and len(exps) - inside >= 30 and 0 in exps
    assert same_bytes(lo4, lo8) and same_bytes(g4, g8)
    lo3, g3, _ = step({"CMLPL_F16X2": "0"})
    assert not same_bytes(g4, g3), "the two-piece loops did not run in the four-wave step"
