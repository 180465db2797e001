"""The loss-block regime table: one case per regime of the loss block (csrc/loss.hip), the switches a case runs under and
the plan the library must then report (cmlpl_debug_loss_plan: host arithmetic, no device).  Plain data plus a reader of
that plan, the input generator and the fp64 conditions every case's inputs must meet:
tests/test_gpu_loss_envelope.py runs the runs on the GPU against the fp64 oracle, tests/test_loss_plan_cpu.py holds the
planner to the same table without a device.

Every case: bank pointers (Q - 5, 3), so bank 0's write wraps; Q >= bt + btu; btu <= 2048.  The shapes are the smallest at
which the regime exists.  Plans that depend on the compute-unit count (`cu_dep`) are stated for 256 units."""
import ctypes as C
from typing import NamedTuple

PAIR16, PAIR32, TALL, WIDE = 0, 1, 2, 3          # LOSS_* of csrc/kernels.hpp
KERNELS = {PAIR16: "pair_exp16_kernel", PAIR32: "pair_exp_kernel", TALL: "pair_exp_tall_kernel", WIDE: "pair_exp_wide_kernel"}
BOTH_EPILOGUES = (PAIR32, TALL)                  # kernels with an LDS epilogue (K <= 32) and a shuffle epilogue (K > 32)
WIDE_SHAPES = ((2, 1), (2, 2), (4, 1), (4, 2), (4, 3), (4, 4))      # pair_exp_wide_kernel<MB, 4 / MB, NBW> as instantiated
SWITCHES = ("CMLPL_PAIR_WIDE", "CMLPL_PAIR_NBW", "CMLPL_PAIR_MB", "CMLPL_PAIR16", "CMLPL_PAIR_TALL", "CMLPL_DFEAT_LDS")
MARGIN = 1e-4                                    # fp64 margin of every deciding comparison: 1000 x fp32's rounding of a probability


class Plan(NamedTuple):
    kernel: int; MB: int; NBW: int; gx: int; gy: int; ctiles: int
    lds_shape: bool     # the shape allows the LDS feature-gradient launch
    lds: bool           # ... and CMLPL_DFEAT_LDS does not forbid it
    cus: int


def read_plan(K, bt, btu, Q, smooth, shard=None):
    from cmlpl_amd import _lib
    out = (C.c_int * 9)()
    sh = _lib.Shard(*(shard or (bt, btu, 0, bt, 0, btu)))
    _lib.check("cmlpl_debug_loss_plan", _lib.load().cmlpl_debug_loss_plan(
        C.byref(_lib.Shape(60, 20, 20, 103, K)), C.byref(sh), Q, int(smooth), out))
    o = list(out)
    return Plan(*o[:6], bool(o[6]), bool(o[7]), o[8])


class Case(NamedTuple):
    name: str
    bt: int; btu: int; K: int; Q: int
    smooth: bool
    adap: float         # adap_mask
    scale: float        # logits = scale x N(0, 1); the second network's = the first's + 0.3 x noise
    seed: int           # walked on the CPU until every deciding comparison has MARGIN in fp64 (check_conditions)
    lds_shape: bool     # rows in whole 16-byte pieces: the LDS feature-gradient launch by shape
    why: str


class Run(NamedTuple):
    case: Case
    env: dict           # the CMLPL_* switches the run is made under ({}: the defaults)
    kernel: int; MB: int; NBW: int; gx: int; gy: int     # the expected plan
    cu_dep: bool        # the plan holds on 256 compute units (asserted only there)
    why: str

    @property
    def id(self):
        sw = "-".join(f"{k[6:]}={v}" for k, v in self.env.items()) or "default"
        return f"{self.case.name}-{sw}"

    @property
    def lds(self):
        return self.case.lds_shape and self.env.get("CMLPL_DFEAT_LDS") != "0"


def _c(name, bt, btu, K, Q, smooth, adap, scale, seed, why):
    return Case(name, bt, btu, K, Q, smooth, adap, scale, seed, btu % 4 == 0, why)


K32 = _c("k32", 20, 44, 32, 256, True, 0.6, 9.0, 1, "16-row kernel at the last K of the LDS epilogue (pw[c * 33 + 31])")
K33 = _c("k33", 24, 40, 33, 256, True, 0.6, 9.0, 1, "32-row kernel, shuffle epilogue, at its first K")
K64 = _c("k64", 16, 48, 64, 200, True, 0.5, 10.0, 1, "32-row kernel, shuffle epilogue, every lane a class; the last column tile holds 8 columns")
K1 = _c("k1", 8, 24, 1, 80, True, 0.9, 8.0, 1, "one-lane softmax: every probability is 1")
ROWS23 = _c("rows23", 9, 23, 2, 90, False, 0.7, 8.0, 1, "rows not a multiple of 4: the direct-load feature-gradient launch by shape; smoothing off (the bank products return early)")
ONE = _c("one", 7, 1, 2, 40, True, 0.7, 8.0, 1, "one unlabelled row: a 1 x 1 pseudo-label graph, both feature-gradient GEMMs with M or R = 1")
T127 = _c("tiles127", 16, 16, 9, 4060, True, 0.6, 9.0, 1, "127 column tiles: still the 16-row kernel")
T128 = _c("tiles128", 16, 16, 9, 4070, True, 0.6, 9.0, 1, "128 column tiles: the wide kernel by the planner, 64 x 64 tiles; the last tile holds 6 columns")
WIDE4 = _c("wide4", 28, 100, 9, 6144, True, 0.6, 9.0, 3, "the planner's wide launch with MB = 4 (2 n64 > 3 CUs on 256 units), two column blocks per wave")
TALL136 = _c("tall136", 24, 136, 9, 4096, True, 0.6, 9.0, 2, "the planner's tall kernel, LDS epilogue; the second row block holds 8 rows")
TALL40 = _c("tall-k40", 16, 72, 40, 4070, True, 0.6, 9.0, 1, "the planner's tall kernel, shuffle epilogue; the third wave partly live, the fourth returns early")

CASES = [K32, K33, K64, K1, ROWS23, ONE, T127, T128, WIDE4, TALL136, TALL40]


def _r(case, env, kernel, MB, NBW, gx, gy, why=None, cu_dep=False):
    return Run(case, env, kernel, MB, NBW, gx, gy, cu_dep, why or case.why)


DEFAULT = [
    _r(K32, {}, PAIR16, 0, 0, 8, 3),
    _r(K33, {}, PAIR32, 0, 0, 8, 2),
    _r(K64, {}, PAIR32, 0, 0, 7, 2),
    _r(K1, {}, PAIR16, 0, 0, 3, 2),
    _r(ROWS23, {}, PAIR16, 0, 0, 1, 2),
    _r(ONE, {}, PAIR16, 0, 0, 2, 1),
    _r(T127, {}, PAIR16, 0, 0, 127, 1),
    _r(T128, {}, WIDE, 2, 1, 64, 1, cu_dep=True),
    _r(WIDE4, {}, WIDE, 4, 2, 96, 1, cu_dep=True),
    _r(TALL136, {}, TALL, 0, 0, 128, 2),
    _r(TALL40, {}, TALL, 0, 0, 128, 1),
]

_W = lambda mb, nbw: {"CMLPL_PAIR_WIDE": "1", "CMLPL_PAIR_MB": str(mb), "CMLPL_PAIR_NBW": str(nbw)}
FORCED = [
    _r(K33, {"CMLPL_PAIR_TALL": "1"}, TALL, 0, 0, 8, 1, "tall tiles with fewer rows (40) than a workgroup holds, shuffle epilogue"),
    _r(K64, {"CMLPL_PAIR_TALL": "1"}, TALL, 0, 0, 7, 1, "tall tiles with fewer rows (48) than a workgroup holds, shuffle epilogue at K = 64"),
    _r(K32, {"CMLPL_PAIR16": "0"}, PAIR32, 0, 0, 8, 2, "the 32-row kernel's LDS epilogue at its limit"),
    # pair_exp_wide_kernel<MB, 4 / MB, NBW>: MB = 2 has 64 NBW columns per workgroup, MB = 4 has 32 NBW
    _r(K32, _W(2, 1), WIDE, 2, 1, 4, 1, "wide<2, 2, 1> at K = 32"),
    _r(K32, _W(2, 2), WIDE, 2, 2, 2, 1, "wide<2, 2, 2> at K = 32"),
    _r(K32, _W(4, 1), WIDE, 4, 1, 8, 1, "wide<4, 1, 1> at K = 32"),
    _r(K32, _W(4, 2), WIDE, 4, 2, 4, 1, "wide<4, 1, 2> at K = 32"),
    _r(K32, _W(4, 3), WIDE, 4, 3, 3, 1, "wide<4, 1, 3> at K = 32"),
    _r(K32, _W(4, 4), WIDE, 4, 4, 2, 1, "wide<4, 1, 4> at K = 32"),
    _r(K33, {"CMLPL_PAIR_WIDE": "1"}, PAIR32, 0, 0, 8, 2, "the wide kernels are refused for K > 32: the plan must say so"),
    _r(K32, {"CMLPL_DFEAT_LDS": "0"}, PAIR16, 0, 0, 8, 3, "the direct-load feature-gradient launch on a shape that allows the LDS one"),
]
RUNS = DEFAULT + FORCED


def check_plan(run, plan):
    """the plan must be the run's regime (asserted before any number is compared); -> whether it was asserted"""
    c = run.case
    maxc = c.Q if (c.smooth and c.Q > c.btu) else c.btu
    assert plan.ctiles == (maxc + 31) // 32, plan
    assert plan.lds_shape == c.lds_shape and plan.lds == run.lds, plan
    if run.cu_dep and plan.cus != 256:
        print(f"[{run.id}] planned for {plan.cus} compute units, not asserted: {plan}")
        return False
    assert (plan.kernel, plan.MB, plan.NBW, plan.gx, plan.gy) == (run.kernel, run.MB, run.NBW, run.gx, run.gy), (run.id, plan)
    return True


# ---- inputs and what must hold of them
def make_inputs(case):
    """float32 inputs of the case: logits and l2-normalised embeddings of both networks, labels, both banks"""
    import torch
    from oracle import cmlpl_oracle as O
    g = torch.Generator().manual_seed(case.seed)
    n, K, Q = case.bt + case.btu, case.K, case.Q
    z0 = torch.randn(n, K, generator=g) * case.scale
    z = [z0, z0 + 0.3 * torch.randn(n, K, generator=g)]      # the networks agree on many rows: Q0 crosses pos_thr
    f = [O.l2norm(torch.relu(torch.randn(n, 1024, generator=g))) for _ in range(2)]
    Y = torch.randint(0, K, (case.bt,), generator=g)
    bf = [O.l2norm(torch.relu(torch.randn(Q, 1024, generator=g))) for _ in range(2)]
    bp = [torch.softmax(torch.randn(Q, K, generator=g) * 3, 1) for _ in range(2)]
    return z, f, Y, bf, bp


def oracle(case, inputs, dtype):
    """O.loss_block in `dtype` with the gradients autograd gives -> (its dict, the tensors under comparison)"""
    import torch
    from oracle import cmlpl_oracle as O
    z, f, Y, bf, bp = inputs
    c = lambda t: t.to(dtype)
    zr = [c(t).clone().requires_grad_(True) for t in z]
    fr = [c(t).clone().requires_grad_(True) for t in f]
    lb = O.loss_block(zr[0], fr[0], zr[1], fr[1], Y, case.bt, [c(t) for t in bf], [c(t) for t in bp], case.smooth,
                      case.adap, O.HyperParams())
    gs = torch.autograd.grad(lb["total_s"], [zr[0], fr[0]], allow_unused=True)
    gw = torch.autograd.grad(lb["total_w"], [zr[1], fr[1]], allow_unused=True)
    zero = lambda t, like: t if t is not None else torch.zeros_like(like)
    out = {k: lb[k].detach().reshape(1) for k in ("ctr_s", "total_s", "cls_s", "con_s", "acc", "total_w", "cls_w", "con_w", "ctr_w")}
    out.update({k: lb[k] for k in ("p_w", "p_s", "p_w0", "p_s0")})
    out.update(dlogits_s=zero(gs[0], zr[0]), dlogits_w=zero(gw[0], zr[1]), dfeat_s=zero(gs[1], fr[0]), dfeat_w=zero(gw[1], fr[1]))
    for i, rows in enumerate((lb["bank0_rows"], lb["bank1_rows"])):
        ep = c(bp[i]).clone()
        O.bank_write(ep, bank_ptr(case)[i], rows[1])
        out[f"bank{i}_probs"] = ep
    return lb, {k: v.detach() for k, v in out.items()}


def bank_ptr(case):
    return (case.Q - 5, 3)          # bank 0's write wraps around the end


def bank_feats_after(case, inputs):
    """the banks' feature rows after the write: a copy of float32 rows, to be met bit for bit"""
    import torch
    from oracle import cmlpl_oracle as O
    z, f, Y, bf, bp = inputs
    bt = case.bt
    out = []
    for i, rows in enumerate((torch.cat([f[1][bt:], f[0][:bt]]), torch.cat([f[0][bt:], f[1][:bt]]))):    # [fU_w ; fL_s], [fU_s ; fL_w]
        ef = bf[i].clone()
        O.bank_write(ef, bank_ptr(case)[i], rows)
        out.append(ef)
    return out


def check_conditions(case, inputs, lb):
    """what the fp64 oracle's run (lb) must show before a device is touched: every comparison that decides something has
    MARGIN, and the decisions are not trivial -> the margins and counts, for the log"""
    import torch
    from oracle import cmlpl_oracle as O
    hp = O.HyperParams()
    btu, K = case.btu, case.K
    assert lb["p_w"].dtype == torch.float64
    m_mask = min(float((lb[k].max(1)[0] - case.adap).abs().min()) for k in ("p_w", "p_s"))
    Q0 = lb["p_s"] @ lb["p_w"].t()
    off = ~torch.eye(btu, dtype=torch.bool)
    m_graph = min(float((Q0[off] - t).abs().min()) for t in (hp.pos_thr, hp.neg_thr)) if btu > 1 else float("inf")
    zl = inputs[0][1][:case.bt].double()                         # the labelled logits `acc` reads (Base1)
    m_acc = float((lambda t: (t[:, 0] - t[:, 1]).min())(zl.topk(2, 1)[0])) if K >= 2 else float("inf")
    got = dict(mask=m_mask, graph=m_graph, acc=m_acc, n_mask_w=int(lb["mask_w"].sum()), n_mask_s=int(lb["mask_s"].sum()),
               n_pos=int(lb["n_pos"]), n_neg=int(lb["n_neg"]))
    assert min(m_mask, m_graph, m_acc) >= MARGIN, (case.name, got)
    if case.smooth and K >= 2 and btu > 1:
        assert any(0 < got[k] < btu for k in ("n_mask_w", "n_mask_s")), (case.name, got)
        assert got["n_pos"] > btu and got["n_neg"] >= 1, (case.name, got)
    return got
