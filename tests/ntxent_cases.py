"""The case table of csrc/ntxent.hip (cmlpl_ntxent_fwd_bwd): one run per edge of its three kernels, the switches a run is
made under, the plan the library must then report (cmlpl_debug_ntxent_plan: host arithmetic, no device), the input
families, the fp64 / fp32 reference, the per-row metric and the conditions the inputs must meet before a device is
touched.  Plain data and CPU code: tests/test_gpu_ntxent_envelope.py runs the runs on the GPU, tests/test_ntxent_plan_cpu.py
holds the planner, the reference and the inputs to the same table without a device.

THE REFERENCE is the loss in matmul form -- x / max(|x|, 1e-12), z z^T, exp with the diagonal masked,
log(den) - S_pos / T, mean -- with autograd for the gradients, evaluated in fp64 and in fp32 (oracle.ntxent_loss builds a
[2B, 2B, D] broadcast: it is tied to this form once, in fp64, and is too slow for a table).

THE METRIC.  x = [emb_i; emb_j] in fp64, n_a = max(|x_a|, 1e-12), E, den, p(a) as in the header of ntxent.hip,
    A_ab = (E_ab (1 / den_a + 1 / den_b) + 2 [b = p(a)]) / (2B T)  for b != a,      s_a = sum_b A_ab / n_a :
the magnitudes of the terms of dz_a = sum_b W_ab z_b, pulled back through the normalisation -- the forward-error scale of
row a's gradient, never zero (also where the gradient is: B = 1, D = 1).
    gradient error = max over rows a and columns d of |got - ref64| / s_a          loss error = |got - ref64| / max(1, |ref64|)
It is per row: a short row (a large gradient) cannot hide the others.

THE BOUND, per quantity: max(BOUND, 8 d32) max(1, 0.5 / T).  BOUND = 2e-6 of the shape envelope, d32 the fp32 reference's
own error in the same metric on the same case, 8 the factor of tests/test_gpu_labelprop.py.  The temperature factor is
derived: a similarity carries an absolute rounding error that does not depend on T and every exponent multiplies it by
1 / T; BOUND was set for the reference's T = 0.5."""
import ctypes as C
import functools
from typing import NamedTuple

import numpy as np
import torch

from tests.test_gpu_shape_envelope import BOUND

VECTOR, MFMA = 0, 1                                # NTX_* of csrc/kernels.hpp
SWITCHES = ("CMLPL_NTX_MFMA", "CMLPL_NTX_NCW")
E_ARG = -1
PLAN_INTS = 10
LDS_MAX, LDS_VECTOR = 160 * 1024, 64 * 1024        # csrc/kernels.hpp; the vector kernel's own limit


def ntxent_plan(B, D, aligned):
    from cmlpl_amd import _lib
    out = (C.c_int * PLAN_INTS)()
    rc = _lib.load().cmlpl_debug_ntxent_plan(B, D, int(aligned), out)
    return rc if rc else tuple(out)


def mfma_lds(N2, ncw):
    """dynamic LDS bytes of ntx_grad_mfma_kernel: iden[N2] | inrm[N2] | red[128] (rounded up to 4 floats) | Wt[N2p][16] |
    xs[2][KC][64 NCW + 16]"""
    N2p, kc = -(-N2 // 64) * 64, 32 if ncw == 4 else 64
    return (((2 * N2 + 128 + 3) & ~3) + 16 * N2p + 2 * kc * (64 * ncw + 16)) * 4


def vector_lds(N2):
    """dynamic LDS bytes of ntx_grad_kernel: iden[N2] | W[8][N2] | red[64] | inrm[N2]"""
    return (10 * N2 + 64) * 4


def full_plan(B, D, route, ncw):
    """the ten integers of cmlpl_debug_ntxent_plan for a route and slice width: the launch geometry restated from the
    kernels' headers (16 x 32 similarity tiles; 8 rows x 256 columns / 16 rows x 64 NCW columns per gradient workgroup)"""
    N2 = 2 * B
    ct = -(-N2 // 32)
    if route == VECTOR:
        return (VECTOR, 0, 0, 4, ct, -(-N2 // 16), -(-N2 // 8), -(-D // 256), vector_lds(N2), ct)
    return (MFMA, ncw, 32 if ncw == 4 else 64, 8 if ncw == 4 else 4, ct, -(-N2 // 16), -(-N2 // 16), -(-D // (64 * ncw)),
            mfma_lds(N2, ncw), ct)


# ============================================================================================ inputs
class Case(NamedTuple):
    name: str
    B: int; D: int
    T: float
    family: str         # "a" .. "g" (below)
    env: tuple          # ((switch, value), ...) the run is made under
    offs: tuple         # (floats emb_i starts past a 16-byte boundary, the same for emb_j)
    route: int
    ncw: int
    why: str

    @property
    def key(self):
        return (self.family, self.B, self.D, self.T)

    @property
    def aligned(self):
        return self.D % 4 == 0 and self.offs == (0, 0)


def _seed(family, B, D):
    return 9000 + 131 * B + 7 * D + ord(family)


def inputs(family, B, D):
    """emb_i, emb_j [B, D] float32 of a family (seeded PCG64, as tests/test_ntxent.py draws them):
      a  N(0, 1) and 2 N(0, 1) + 0.3                           b  row magnitudes 10^linspace(-6, 3, B), reversed on emb_j
      c  one all-zero row in emb_i                              d  two equal rows inside emb_i
      e  emb_j = emb_i       f  emb_j = -emb_i                  g  emb_j = emb_i + 0.1 noise"""
    rng = np.random.Generator(np.random.PCG64(_seed(family, B, D)))
    ei = rng.standard_normal((B, D))
    ej = rng.standard_normal((B, D)) * 2 + 0.3
    if family == "b":
        mag = 10.0 ** np.linspace(-6, 3, B)
        ei, ej = ei * mag[:, None], ej * mag[::-1, None]
    elif family == "c":
        ei[B // 4] = 0.0
    elif family == "d":
        ei[(3 * B) // 4] = ei[B // 8]
    elif family == "e":
        ej = ei.copy()
    elif family == "f":
        ej = -ei
    elif family == "g":
        ej = ei + 0.1 * rng.standard_normal((B, D))
    else:
        assert family == "a", family
    return torch.from_numpy(ei.astype(np.float32)), torch.from_numpy(ej.astype(np.float32))


# ============================================================================================ reference and metric
def reference(ei, ej, T, dtype):
    """loss, d loss / d emb_i, d loss / d emb_j and the denominators, evaluated in `dtype`: every value is a `dtype`
    number and every operation is rounded to `dtype` once -- a reduction (the norms, the products z z^T, the denominators,
    the mean, and their transposes in the backward) is summed in double and then rounded, so that the fp32 evaluation
    shows what the rounding of the VALUES costs and not what one summation order among many costs (a plain fp32 matmul
    and sum over 2B = 1664 terms is 6e-7 from fp64 in the metric, this form 8e-8: d32 only tightens what the kernels are
    held to)."""
    B = ei.shape[0]
    xi, xj = ei.to(dtype).clone().requires_grad_(True), ej.to(dtype).clone().requires_grad_(True)
    x = torch.cat([xi, xj])
    n = x.double().norm(dim=1).to(dtype).clamp_min(1e-12)          # F.normalize: x / max(|x|, 1e-12)
    z = x / n[:, None]
    S = (z.double() @ z.double().T).to(dtype)
    E = torch.exp(S / T).masked_fill(torch.eye(2 * B, dtype=torch.bool), 0.0)
    den = E.double().sum(1).to(dtype)
    pos = torch.cat([torch.diagonal(S, B), torch.diagonal(S, -B)])
    loss = (torch.log(den) - pos / T).double().mean().to(dtype)
    loss.backward()
    return dict(loss=loss.detach().reshape(1), grad_i=xi.grad, grad_j=xj.grad), den.detach()


def row_scale(ei, ej, T):
    """s_a of the metric, [2B] fp64"""
    B = ei.shape[0]
    x = torch.cat([ei, ej]).double()
    n = x.norm(dim=1).clamp_min(1e-12)
    z = x / n[:, None]
    eye = torch.eye(2 * B, dtype=torch.bool)
    E = torch.exp((z @ z.T) / T).masked_fill(eye, 0.0)
    iden = 1.0 / E.sum(1)
    A = E * (iden[:, None] + iden[None, :])
    a = torch.arange(2 * B)
    A[a, (a + B) % (2 * B)] += 2.0
    return A.masked_fill(eye, 0.0).sum(1) / (2 * B * T) / n


def errors(got, ref, scale):
    """the metric of the three quantities: got / ref dicts of loss [1], grad_i, grad_j [B, D]"""
    B = ref["grad_i"].shape[0]
    out = {"loss": float((got["loss"].double() - ref["loss"]).abs() / ref["loss"].abs().clamp_min(1.0))}
    for k, s in (("grad_i", scale[:B]), ("grad_j", scale[B:])):
        out[k] = float(((got[k].double() - ref[k]).abs() / s[:, None]).max())
    return out


def bounds(d32, T):
    return {k: max(BOUND, 8 * d32[k]) * max(1.0, 0.5 / T) for k in d32}


@functools.lru_cache(maxsize=3)
def prepared(key):
    """(emb_i, emb_j), the fp64 reference, the row scales and the fp32 reference's own error, for the inputs of a case --
    built once, shared by the runs of those inputs (the table keeps them adjacent), never written to.  The conditions are
    asserted here, on the CPU:
      * the fp32 and the fp64 reference agree within BOUND / 8 in both metrics (the inputs are well conditioned: a
        saturated loss is not -- near-duplicate views at T = 0.05 give a loss of 1e-6 with 40 % fp32 error);
      * every fp32 denominator is finite;
      * the loss exceeds 1e-3 (B = 1 has loss 0 by definition: its only negative is its positive)."""
    family, B, D, T = key
    ei, ej = inputs(family, B, D)
    ref, _ = reference(ei, ej, T, torch.float64)
    ref32, den32 = reference(ei, ej, T, torch.float32)
    scale = row_scale(ei, ej, T)
    assert bool((scale > 0).all()) and bool(torch.isfinite(scale).all())
    d32 = errors(ref32, ref, scale)
    assert max(d32.values()) <= BOUND / 8, (key, d32)
    assert bool(torch.isfinite(den32).all()), key
    assert B == 1 or float(ref["loss"]) > 1e-3, (key, float(ref["loss"]))
    return (ei, ej), ref, scale, d32


# ============================================================================================ the table
# Where the planner's own thresholds and the capacity limits lie (derived in tests/test_ntxent_plan_cpu.py):
NCW2_FIRST, NCW4_FIRST = (249, 900), (505, 772)    # the first (B, D) of 128- and of 256-column slices
LAST_VECTOR, LAST_MFMA = 816, 832                  # the last B each route holds (2B = 1632, 1664)


def _build():
    cases = []

    def add(name, B, D, why, T=0.5, family="a", env=(), offs=(0, 0), route=None, ncw=None):
        env = tuple(env)
        aligned = D % 4 == 0 and offs == (0, 0)
        if route is None:
            route = MFMA if aligned and ("CMLPL_NTX_MFMA", "0") not in env else VECTOR
        if ncw is None:
            ncw = 0 if route == VECTOR else int(dict(env).get("CMLPL_NTX_NCW", 1))
        cases.append(Case(name, B, D, T, family, env, offs, route, ncw, why))

    # ---- the row tiles: 2B around 8 (NTX_R), 16 / 32 (the similarity tile), 64 (N2p), on both gradient kernels
    for B in (1, 2, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33):
        for D in (36, 37):
            add(f"rows-b{B}-d{D}", B, D, f"2B = {2 * B}: row / column tiles of 8, 16, 32, 64 on the "
                f"{'MFMA' if D == 36 else 'vector'} kernel")
    # ---- the contraction and the column slices at B = 9
    for D in (1, 2, 3, 4, 5, 31, 32, 33, 60, 64, 68, 96, 100, 127, 128, 129, 132, 255, 256, 257, 260):
        add(f"cols-d{D}", 9, D, "D < 4; 32-float lines of the four waves (D <= 96: waves without a line); slices of 64 / "
            "128 / 256 columns; the vector kernel's block of 256")
    # ---- the chunk pipeline: 1 .. 5 chunks of 64 rows (2 .. 10 of 32 at NCW = 4), whole and ragged column slices
    for D in (260, 64):
        for B in (32, 33, 64, 65, 96, 97, 128, 129, 160):
            for ncw in (1, 2, 4):
                kc = 32 if ncw == 4 else 64
                add(f"chunks-b{B}-d{D}-ncw{ncw}", B, D, f"{-(-2 * B // 64) * 64 // kc} chunks of {kc} rows under a forced slice of {64 * ncw} "
                    f"columns ({-(-D // (64 * ncw))} slices, the last {'ragged' if D % (64 * ncw) else 'whole'})",
                    env=(("CMLPL_NTX_NCW", str(ncw)),))
    # ---- the thread stride of the b loops (256; 512 with eight waves) and the batched partial sums (CT past 8, 32)
    for B in (129, 257, 513):
        add(f"stride-b{B}-d8", B, 8, f"2B = {2 * B} past {2 * (B - 1)}: CT = {-(-2 * B // 32)} (MFMA prologue: 32 partials a trip)")
        add(f"stride-b{B}-d6", B, 6, f"2B = {2 * B} past {2 * (B - 1)}: CT = {-(-2 * B // 32)} (vector prologue: 8 partials a trip)")
    add("stride-b257-d8-ncw4", 257, 8, "2B = 514 past the 512 threads of the eight-wave instantiation",
        env=(("CMLPL_NTX_NCW", "4"),))
    # ---- the planner's own first wide slices (the largest cases)
    add("planner-ncw2", *NCW2_FIRST, "the first shape the planner gives 128-column slices: 32 row groups x 8 slices = 256", ncw=2)
    add("planner-ncw4", *NCW4_FIRST, "the first shape the planner gives 256-column slices: 64 row groups x 4 slices = 256", ncw=4)
    # ---- capacity: the last B of each route
    add("last-mfma", LAST_MFMA, 8, "2B = 1664: the last batch the single-slice MFMA kernel holds in LDS (beyond the vector kernel's)")
    add("last-vector", LAST_VECTOR, 5, "2B = 1632: the vector kernel's 64 KiB of LDS exactly")
    # ---- pointer alignment: D a multiple of 4 but rows that start 4 bytes past a 16-byte boundary
    add("offset-both", 24, 64, "both embedding pointers 4 bytes off: the vector kernel", offs=(1, 1))
    add("offset-i", 24, 64, "emb_i 4 bytes off, emb_j aligned: the vector kernel", offs=(1, 0))
    add("offset-j", 24, 64, "emb_j 4 bytes off, emb_i aligned: the vector kernel", offs=(0, 1))
    # ---- the input families on both kernels
    whys = dict(b="row magnitudes 1e-6 .. 1e3", c="an all-zero row: the eps clamp and the / n of the backward at n = 1e-12",
                d="two equal rows inside emb_i", e="identical views", f="opposite views", g="near-duplicate views, T = 0.2")
    for D in (68, 67):
        for fam in "bcdefg":
            add(f"family-{fam}-d{D}", 24, D, whys[fam], T=0.2 if fam == "g" else 0.5, family=fam)
        for fam in "adf":
            add(f"cold-{fam}-d{D}", 24, D, "T = 0.05: exponents up to 20" + (", " + whys[fam] if fam in whys else ""), T=0.05, family=fam)
    return cases


CASES = _build()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
# refused: the first B past each route (CMLPL_E_ARG before anything is launched)
REFUSED = [(LAST_MFMA + 1, 8, "one past the MFMA kernel's last batch, rows aligned"),
           (LAST_VECTOR + 1, 5, "one past the vector kernel's last batch")]
# inputs run on every route that fits (vector, 64 / 128 / 256-column slices): the routes must agree
ALL_ROUTES = [(33, 260), (97, 64), (160, 260), (257, 8), (24, 68)]
ROUTE_ENVS = [(("CMLPL_NTX_MFMA", "0"),), (("CMLPL_NTX_NCW", "1"),), (("CMLPL_NTX_NCW", "2"),), (("CMLPL_NTX_NCW", "4"),)]
