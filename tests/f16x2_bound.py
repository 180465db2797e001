"""The per-element error bound of the TWO-fp16-piece products (csrc/conv3x3.hip: conv3_taps_ks_h / conv3_taps_h;
csrc/wgrad3x3.hip: wgrad3b_body<.., true>), the fp64 re-computation of a 3x3 stage from the
DEVICE'S OWN operands that the GPU tests compare against, and a CPU emulation of the scheme.  No device, no library:
tests/test_f16x2_bound_cpu.py holds the emulation (and three deliberately wrong ones) to the bound,
tests/test_gpu_f16x2_range.py and tests/test_gpu_ops.py hold the kernels to it.

The bound, derived from the scheme (not from what the kernels give):

* An image (activations in the forward, the masked up-sampled pooled gradient in the backward) is scaled by
  s = 2^(14 - E), E = floor(log2 max|image|) of ITS sample, and split into h1 = fp16(a s) truncated and h2 = fp16 of
  the exact residual, truncated.  While the residual is a normal fp16 the two pieces keep 21 bits (relative error below
  2^-21); fp16's spacing never exceeds 2^-24 below 2^-14, so in every case the value the MFMA sees differs from a s by
  at most max(2^-21 |a s|, 2^-24): an ABSOLUTE error of at most max(2^-21 |a|, 2^-24 / s) = max(2^-21 |a|, 2^(E - 38))
  per activation.  (2^(E - 38) lies between 2^-39 and 2^-38 of the sample's maximum.)
* A weight is scaled by 2^13 and split into two pieces rounded to nearest: relative 2^-22, absolute 2^-25 / 2^13 = 2^-38
  for a weight whose scaled value is below 2^-14.
* The product h2 g2 is dropped: below 2^-22 |a w|.
* The three products of fp16 numbers are exact in the MFMA's fp32 accumulation input; the accumulation and the epilogue
  (bias, residual, ReLU, pool) round as an fp32 dot product does: the project's own constants for that are
  c = 2^-18 of S_i for the 576 terms of a forward / data-gradient element and 2^-16 of S for a weight-gradient element
  (tests/test_gpu_ops.py::test_split_bf16_conv1_error_bound_per_element), and the relative terms above (2^-21 + 2^-22 +
  2^-22 < 2^-20) are inside them as the three-piece loop's 2^-21 is.

Forward and data gradient, element i of sample s:

    |err_i| <= c S_i + u_s W_i + 2^-38 A_i,   S_i = sum |a||w| + |bias| + |residual|,  W_i = sum |w|,  A_i = sum |a|
                                               over the same terms,  u_s = 2^(E_s - 38),  c = 2^-18

(pooled outputs: the bound of the four pre-pool elements, pooled with the device's ReLU decisions, as S is).  Weight
gradient (both operands are images; the scales come from the BATCH maxima):

    |err| <= 2^-16 S + u_a sum |g| + u_g sum |a|,   u_a = 2^(E_a - 38), u_g = 2^(E_g - 38)

`flushed=True` states the bound a device that flushes fp16 subnormals would obey instead (absolute term 2^-14 / s:
u = 2^(E - 28); the weights' 2^-14 / 2^13 = 2^-27).  The kernels are NOT held to it unless that is what the hardware does."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.test_split_f16_math import a_pieces, w_pieces

C_FWD = 2.0 ** -18
C_WGRAD = 2.0 ** -16
U_EXP, U_EXP_FLUSHED = 38, 28        # u = 2^(E - 38); 2^(E - 28) if fp16 subnormals were flushed
W_ABS, W_ABS_FLUSHED = 2.0 ** -38, 2.0 ** -27
E_LO, E_HI, E_SUM = 40, 200, 160     # the exponent fields the two-piece loops accept
ZERO = torch.zeros((), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------- exponents and the rule
def expo(t):
    """exponent field of the largest magnitude of an fp32 tensor, as the kernels take it (bit patterns: NaN / inf -> 255)"""
    t = t.detach().float().cpu()
    if t.numel() == 0:
        return 0
    if torch.isnan(t).any():
        return 255
    return int(t.abs().max().view(torch.int32)) >> 23


def expos(t):
    """expo() per sample (dim 0)"""
    return [expo(t[s]) for s in range(t.shape[0])]


def image_two_piece(t):
    """DESIGN section 4, a sample's image: two-piece when its maximum's exponent field is in 40 .. 200 or the image is zero"""
    e = expo(t)
    return E_LO <= e <= E_HI or not bool((t != 0).any() or torch.isnan(t).any())


def wgrad_two_piece(ea, eg):
    """the weight gradients' rule on the BATCH exponents"""
    return E_LO <= ea <= E_HI and E_LO <= eg <= E_HI and ea + eg >= E_SUM


def u_of(e, flushed=False):
    """the absolute term's factor for exponent field e (0 for an image without an ordinary maximum: nothing to scale)"""
    return 2.0 ** (e - 127 - (U_EXP_FLUSHED if flushed else U_EXP)) if 0 < e < 255 else 0.0


def pow2(q):
    """2^q as an fp32 tensor scalar, exact for -149 <= q <= 127"""
    return torch.tensor(2.0, dtype=torch.float64).pow(q).float()


# ------------------------------------------------------------------------------------- fp64 stages from given operands
def nchw(region, n, h, w):
    """a saved [n][h w][64] fp32 region -> fp64 [n, 64, h, w] on the CPU"""
    return region.view(-1)[: n * h * w * 64].view(n, h * w, 64).cpu().double().permute(0, 2, 1).reshape(n, 64, h, w)


def _pool(x, gate):
    return F.avg_pool2d(torch.where(gate, x, ZERO), 2)


def forward_stage(a, w, b, gate, flushed=False):
    """p = avgpool2(relu(conv3x3(a) + b + a)) in fp64 with GIVEN ReLU decisions, and the pooled pieces of the bound.
    a [n,64,h,w] fp64 (the device's operand), gate bool [n,64,h,w] -> dict p, S, bound (two-piece), plain (c S)."""
    a, w, b = a.double(), w.double(), b.double()
    ones_a, ones_w = torch.ones_like(a[:1]), torch.ones_like(w)
    z = F.conv2d(a, w, b, padding=1) + a
    S = F.conv2d(a.abs(), w.abs(), b.abs(), padding=1) + a.abs()
    Wt = F.conv2d(ones_a, w.abs(), None, padding=1)                    # sum |w| over the taps inside the map
    At = F.conv2d(a.abs(), ones_w, None, padding=1)
    u = torch.tensor([u_of(e, flushed) for e in expos(a)], dtype=torch.float64).view(-1, 1, 1, 1)
    bz = C_FWD * S + u * Wt + (W_ABS_FLUSHED if flushed else W_ABS) * At
    return {"p": _pool(z, gate), "S": _pool(S, gate), "bound": _pool(bz, gate), "plain": C_FWD * _pool(S, gate),
            "abs": _pool(u * Wt + 0 * S, gate)}


def grad_image(dp, gate, H, W):
    """the backward's image: dz = relu'(z) * upsample(dp) / 4 (avgpool + ReLU backward), zero on the last row / column of
    an odd map.  dp [n,64,H/2,W/2] fp64, gate bool [n,64,H,W]."""
    n, H2, W2 = dp.shape[0], H // 2, W // 2
    dz = torch.zeros(n, 64, H, W, dtype=torch.float64)
    dz[:, :, :2 * H2, :2 * W2] = dp.repeat_interleave(2, 2).repeat_interleave(2, 3) / 4
    dz = torch.where(gate, dz, ZERO)
    dz[:, :, 2 * H2:, :] = 0
    dz[:, :, :, 2 * W2:] = 0
    return dz


def dgrad_stage(dz, w, flushed=False):
    """da = conv3x3^T(dz) + dz in fp64 and its bound.  dz: grad_image()."""
    dz, w = dz.double(), w.double()
    H, W = dz.shape[2:]
    sup = torch.zeros_like(dz[:1])                                     # where the image can be non-zero
    sup[:, :, :2 * (H // 2), :2 * (W // 2)] = 1
    da = F.conv_transpose2d(dz, w, padding=1) + dz
    S = F.conv_transpose2d(dz.abs(), w.abs(), padding=1) + dz.abs()
    Wt = F.conv_transpose2d(sup, w.abs(), padding=1)
    At = F.conv_transpose2d(dz.abs(), torch.ones_like(w), padding=1)
    u = torch.tensor([u_of(e, flushed) for e in expos(dz)], dtype=torch.float64).view(-1, 1, 1, 1)
    return {"p": da, "S": S, "bound": C_FWD * S + u * Wt + (W_ABS_FLUSHED if flushed else W_ABS) * At, "plain": C_FWD * S}


def wgrad_stage(a, dz, flushed=False):
    """dW = sum over samples and pixels a(shifted) dz in fp64 and its bound; the scales are the batch's"""
    a, dz = a.double(), dz.double()
    H, W = dz.shape[2:]
    ws = (64, 64, 3, 3)
    sup = torch.zeros_like(dz)
    sup[:, :, :2 * (H // 2), :2 * (W // 2)] = 1
    cw = lambda x, y: torch.nn.grad.conv2d_weight(x, ws, y, padding=1)
    dw, S = cw(a, dz), cw(a.abs(), dz.abs())
    G, A = cw(torch.ones_like(a), dz.abs()), cw(a.abs(), sup)
    ea, eg = expo(a), expo(dz)
    return {"p": dw, "S": S, "bound": C_WGRAD * S + u_of(ea, flushed) * G + u_of(eg, flushed) * A, "plain": C_WGRAD * S,
            "ea": ea, "eg": eg}


def worst(got, st, key="bound"):
    """largest |err| / bound over the elements (0 / 0 counts as 0; a NaN anywhere gives inf)"""
    err = (got.double() - st["p"]).abs()
    r = torch.where(err == 0, ZERO, err / st[key])
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


# ----------------------------------------------------------------------------------------------- the scheme on the CPU
def _flush16(h):
    return np.where(np.abs(h) < 2.0 ** -14, 0.0, h)


def image_scale(x):
    """(hsc, e) of one sample's image (fp32 numpy): hsc = 2^(268 - e)"""
    e = int(np.float32(np.abs(x).max()).view(np.uint32) >> 23)
    assert E_LO <= e <= E_HI, e
    return np.uint32((268 - e) << 23).view(np.float32), e


def emulate_stage(a, w, b, gate=None, wrong=None):
    """The two-piece tap loop on fp32 operands: pieces by tests/test_split_f16_math.py's helpers, the three products
    h1 g1 + h2 g1 + h1 g2 accumulated EXACTLY (fp64), un-scaled by hinv = 1 / (hsc 2^13), + bias + residual; with `gate`
    (the ReLU decisions, bool) also ReLU and the 2 x 2 pool -- a forward stage; without, the data gradient's shape (pass the
    transposed, flipped weights and no bias).  a [n,64,h,w] fp32 torch.  `wrong`: None, or one of the faults the bound
    must catch -- "scale_high": hsc one binade too high (a wrong exponent constant; hinv as the kernel forms it), "no_h2":
    the second activation piece dropped, "flush": fp16 subnormals flushed to zero in every piece."""
    n = a.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        _, g1, g2 = w_pieces(w.numpy().astype(np.float32))
        if wrong == "flush":
            g1, g2 = _flush16(g1), _flush16(g2)
        g1, g2 = torch.from_numpy(g1), torch.from_numpy(g2)
        z = torch.empty(a.shape, dtype=torch.float64)
        bias = torch.zeros(64, dtype=torch.float64) if b is None else b.double()
        for s in range(n):
            x = a[s].numpy().astype(np.float32)
            if not x.any():                                   # a zero image: scale 1, exact zeros
                z[s] = bias.view(64, 1, 1)
                continue
            sc, e = image_scale(x)
            inv = 2.0 ** (e - 154)                            # hinv: 1 / (hsc 2^13)
            if wrong == "scale_high":
                sc = np.float32(sc * np.float32(2.0))
            _, h1, h2 = a_pieces(x, sc)
            if wrong == "no_h2":
                h2 = np.zeros_like(h2)
            if wrong == "flush":
                h1, h2 = _flush16(h1), _flush16(h2)
            h1, h2 = torch.from_numpy(h1)[None], torch.from_numpy(h2)[None]
            acc = F.conv2d(h1, g1, None, padding=1) + F.conv2d(h2, g1, None, padding=1) + F.conv2d(h1, g2, None, padding=1)
            z[s] = acc[0] * inv + bias.view(64, 1, 1) + a[s].double()
    return z if gate is None else _pool(z, gate)


def transposed(w):
    """the data gradient's weights: conv2d(dz, transposed(w)) = conv_transpose2d(dz, w)"""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def emulate_wgrad(a, dz, wrong=None):
    """The two-piece weight gradient on fp32 operands: both images split at the BATCH scales, three products, exact sums"""
    with np.errstate(over="ignore", invalid="ignore"):
        xa, xg = a.numpy().astype(np.float32), dz.numpy().astype(np.float32)
        (sa, ea), (sg, eg) = image_scale(xa), image_scale(xg)
        inv = 2.0 ** (ea + eg - 282)                          # the kernel's 2^(ea + eg - 155) as a field: 1 / (sa sg)
        assert float(sa) * float(sg) * inv == 1.0
        if wrong == "scale_high":
            sa = np.float32(sa * np.float32(2.0))
        _, a1, a2 = a_pieces(xa, sa)
        _, d1, d2 = a_pieces(xg, sg)
        if wrong == "no_h2":
            a2 = np.zeros_like(a2)
        if wrong == "flush":
            a1, a2, d1, d2 = _flush16(a1), _flush16(a2), _flush16(d1), _flush16(d2)
        t = torch.from_numpy
        cw = lambda x, y: torch.nn.grad.conv2d_weight(t(x), (64, 64, 3, 3), t(y), padding=1)
        return (cw(a1, d1) + cw(a2, d1) + cw(a1, d2)) * inv


# ------------------------------------------------------------------------------------------------------ the test inputs
K_GROUPS = (0, 12, 16, 17, 18, 20, 24, 28)     # conv0's output channels 8 g .. 8 g + 7 are scaled by 2^-K_GROUPS[g]
SMALL_FROM = {1: 24, 2: 32}                    # conv1's output channels 16 .. 31 read the input channels of k >= 17 only,
                                               # 32 .. 63 those of k >= 18 only


def channel_k():
    return torch.tensor([K_GROUPS[c // 8] for c in range(64)])


def wide_range_params(params):
    """Section 3b: a wide range INSIDE one sample on the two-piece path.  conv0's output channels fall off by 2^-k in eight
    groups (NOT undone in conv1); conv1's output channels 16 .. 31 read only the input channels at k >= 17 and 32 .. 63
    only those at k >= 18, with weights up to ~4 (96 x the closed-form ones: max |w| 2^13 stays below 65000, the range flag
    stays clear), so that those outputs have no large term to hide an absolute error behind; their bias falls off like
    the channel's residual.  Powers of two throughout: the scaling itself does not round."""
    p = {k: v.clone() for k, v in params.items()}
    sc = torch.tensor(2.0).pow(-channel_k().float())
    p["conv0.weight"] = p["conv0.weight"] * sc.view(64, 1, 1, 1)
    p["conv0.bias"] = p["conv0.bias"] * sc
    w1 = p["conv1.weight"].clone()
    w1[16:32, :SMALL_FROM[1]] = 0
    w1[32:64, :SMALL_FROM[2]] = 0
    w1[16:64] = w1[16:64] * 96.0
    p["conv1.weight"] = w1
    b1 = p["conv1.bias"].clone()
    b1[16:] = b1[16:] * sc[16:] * 2.0 ** -12
    p["conv1.bias"] = b1
    return p


def no_conv_bias(params, keys=("conv0.bias", "conv1.bias", "conv2.bias")):
    """without the convolutions' biases the stages are homogeneous: scaling a sample's input by 2^q scales its images
    exactly (conv0 is a 1x1 convolution without ReLU) and leaves its ReLU decisions alone"""
    return {k: (torch.zeros_like(v) if k in keys else v.clone()) for k, v in params.items()}


def inputs(shape, n, seed):
    """x [n,C,H,W], y [n,bands], dlog [n,K] of a test batch (shape: anything with C, H, W, bands, K)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, shape.C, shape.H, shape.W, generator=g), torch.randn(n, shape.bands, generator=g),
            torch.randn(n, shape.K, generator=g))


def oracle_images(p, x, y, dlog):
    """The fp32 oracle's operands of the four two-piece loops and the weight gradients: the forward of
    oracle.cmlpl_oracle.basenet2_forward spelled out so that the images can be kept (the logits are compared with its),
    the gradient images dz1 / dz2 by autograd.  -> dict a0, p1, gate1, gate2, dz1, dz2 (fp32), logits"""
    w1, b1, w2, b2 = p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"]
    a0 = F.conv2d(x, p["conv0.weight"], p["conv0.bias"])
    z1 = (F.conv2d(a0, w1, b1, padding=1) + a0).requires_grad_()
    p1 = F.avg_pool2d(F.relu(z1), 2, 2)
    z2 = F.conv2d(p1, w2, b2, padding=1) + p1
    z2.retain_grad()
    t = F.avg_pool2d(F.relu(z2), 2, 2).reshape(x.shape[0], -1)
    ys = F.relu(F.linear(y, p["feat_spe.weight"], p["feat_spe.bias"]))
    logits = F.linear(torch.cat([t, ys], 1), p["classifier.weight"], p["classifier.bias"])
    (logits * dlog).sum().backward()
    return {"a0": a0.detach(), "p1": p1.detach(), "gate1": z1.detach() > 0, "gate2": z2.detach() > 0,
            "dz1": z1.grad.detach(), "dz2": z2.grad.detach(), "logits": logits.detach()}
