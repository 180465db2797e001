"""The regime tables of csrc/memobank.hip: one case per route of the entropy-filtered cross entropy (cmlpl_unsup_loss)
and per regime of the memory-bank InfoNCE in one pass (cmlpl_memobank_loss), the switches a run is made under, the plan
the library must then report (cmlpl_debug_unsup_plan / cmlpl_debug_memobank_plan: host arithmetic, no device), the input
builders and the conditions the inputs must meet before a device is touched.  Plain data and CPU code:
tests/test_gpu_memobank_envelope.py runs the runs on the GPU against the fp64 oracle, tests/test_memobank_plan_cpu.py
holds the two planners and the inputs to the same tables without a device."""
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from oracle import cmlpl_oracle as O

ONEWG, THREE, FIVE = 0, 1, 2                       # US_* of csrc/kernels.hpp
ROUTES = {ONEWG: "us_onewg_kernel", THREE: "us_entropy2_kernel + us_select1_kernel + us_apply_kernel",
          FIVE: "us_entropy_kernel + us_rank_kernel + us_select_kernel + us_mask_kernel + us_grad_kernel"}
SWITCHES = ("CMLPL_UNSUP_ONEWG", "CMLPL_UNSUP_3L", "CMLPL_MB_FAST")
E_ARG = -1
MARGIN_ULPS = 64                                   # decisions: 64 x the fp32 oracle's own entropy error away from the threshold


def unsup_plan(B, K):
    from cmlpl_amd import _lib
    out = (C.c_int * 2)()
    rc = _lib.load().cmlpl_debug_unsup_plan(B, K, out)
    return rc if rc else (out[0], out[1])


def memobank_plan(D, K, Q, NN):
    from cmlpl_amd import _lib
    out = (C.c_int * 3)()
    rc = _lib.load().cmlpl_debug_memobank_plan(D, K, Q, NN, out)
    return rc if rc else (out[0], out[1], out[2])


# ============================================================================================ cmlpl_unsup_loss
class UCase(NamedTuple):
    name: str
    B: int; K: int
    percent: float
    seed: int
    ignored: int        # rows that are 255 from the start (variant a)
    variant: str        # "" | "tie_in" | "tie_lo" | "tie_above" (variant b i / ii / iii) | "n1" | "n2" (variant c)
    g: str              # what the fraction of the virtual index must be: "" (any) | "zero" | "low" (0 < g < 0.5) | "high"
    why: str


TIE_ROWS = 4            # m of the tie block

UCASES = [
    UCase("b1-k9", 1, 9, 50.0, 11, 0, "", "zero", "one row: it is its own percentile and is dropped, nothing is kept"),
    UCase("b63-k2", 63, 2, 37.0, 12, 5, "", "", "one partial wave of the one workgroup, two classes"),
    UCase("b65-k16", 65, 16, 80.0, 13, 3, "tie_lo", "", "one row past a wave; the register row full (K = 16); a[lo] the tie block, a[hi] the next value"),
    UCase("b255-k9", 255, 9, 60.0, 14, 9, "tie_above", "", "the rank kernel's only column slice partly filled, fifteen slices without rows"),
    UCase("b257-k9", 257, 9, 25.0, 15, 7, "tie_in", "", "two row blocks of the rank kernel, the second with one row"),
    UCase("b1024-k9", 1024, 9, 100.0, 16, 21, "", "zero", "every thread of the one workgroup a row; percent 100: only the maximum goes"),
    UCase("b1024-k16", 1024, 16, 45.0, 17, 0, "tie_in", "", "the last B of one row per thread at K = 16; a[lo] and a[hi] inside the tie block"),
    UCase("b1024-k17", 1024, 17, 70.0, 18, 30, "", "", "the first K of the per-k loops"),
    UCase("b1025-k9", 1025, 9, 20.0, 19, 40, "tie_in", "", "the first B of three launches / two rows per thread; a[lo] and a[hi] inside the tie block"),
    UCase("b1025-k17", 1025, 17, 66.0, 20, 12, "tie_lo", "", "three launches, per-k loops; a[lo] the tie block, a[hi] the next value"),
    UCase("b1025-g0", 1025, 9, 25.0, 21, 924, "", "zero", "101 valid rows at percent 25: an integral virtual index"),
    UCase("b1025-n1", 1025, 9, 50.0, 22, 1024, "n1", "zero", "one valid row: dropped, nothing is kept"),
    UCase("b1025-n2", 1025, 9, 50.0, 23, 1023, "n2", "high", "two valid rows at percent 50: g = 0.5, the upper one goes"),
    UCase("b8192-k16", 8192, 16, 33.0, 24, 100, "tie_above", "high", "the last B of three launches / eight rows per thread; the tie block wholly above a[hi]; g >= 0.5"),
    UCase("b8192-k17", 8192, 17, 100.0, 25, 64, "", "zero", "eight rows per thread in the per-k loops; percent 100"),
    UCase("b8192-k9", 8192, 9, 36.0, 26, 700, "", "low", "eight rows per thread, register rows, 0 < g < 0.5"),
    UCase("b8193-k9", 8193, 9, 40.0, 27, 50, "tie_lo", "", "the first B only the five launches take; sixteen column slices of 768 rows, the last with 1"),
    UCase("b8193-k17", 8193, 17, 55.0, 28, 0, "tie_in", "", "the largest batch of the table; ties by row index in the rank kernel"),
]

DEGENERATE = [   # (B, K, percent, all rows ignored): nothing kept -- not held to the oracle (autograd gives NaN gradients)
    (300, 9, 0.0, False), (300, 9, 50.0, True), (2000, 17, 0.0, False), (2000, 9, 50.0, True), (8193, 9, 0.0, False),
]


class URun(NamedTuple):
    case: UCase
    env: dict
    route: int
    regrows: int
    why: str

    @property
    def id(self):
        return f"{self.case.name}-" + ("-".join(f"{k[6:]}={v}" for k, v in self.env.items()) or "default")


def unsup_routes(B, K):
    """every route a batch of B rows can take, with the switches that force it: [(env, route, regrows)]"""
    rr = 1 if K <= 16 else 0
    if B <= 1024:
        return [({}, ONEWG, rr), ({"CMLPL_UNSUP_ONEWG": "0"}, FIVE, 0)]
    if B <= 8192:
        return [({}, THREE, rr), ({"CMLPL_UNSUP_3L": "0"}, ONEWG, rr), ({"CMLPL_UNSUP_ONEWG": "0"}, FIVE, 0)]
    return [({}, FIVE, 0)]


def _uwhy(case, route, rr):
    body = "" if route == FIVE else (", register rows" if rr else ", per-k loops")
    rows = f", {-(-case.B // 1024)} rows per thread" if route == ONEWG and case.B > 1024 else ""
    return f"{ROUTES[route]}{body}{rows}: {case.why}"


URUNS = [URun(c, env, route, rr, _uwhy(c, route, rr)) for c in UCASES for env, route, rr in unsup_routes(c.B, c.K)]


def _entropy(teacher):
    p = torch.softmax(teacher, dim=1)
    return -(p * torch.log(p + 1e-10)).sum(dim=1)


def unsup_order(teacher, target, percent):
    """fp64 view of one batch: entropies, the valid rows sorted by (entropy, row), lo, hi, g, the threshold, and
    MARGIN_ULPS x the fp32 oracle's largest entropy error on the valid rows"""
    e64, e32 = _entropy(teacher.double()), _entropy(teacher.float())
    valid = (target != O.IGNORE).nonzero().flatten()
    n = int(valid.numel())
    order = valid[np.lexsort((valid.numpy(), e64[valid].numpy()))]
    vidx = (n - 1) * percent / 100.0
    lo = int(np.floor(vidx))
    hi = min(lo + 1, n - 1)
    thr = float(np.percentile(e64[valid].numpy(), percent))
    eps = MARGIN_ULPS * float((e32[valid].double() - e64[valid]).abs().max())
    return dict(e64=e64, order=order, n=n, lo=lo, hi=hi, g=vidx - lo, thr=thr, eps=eps)


def unsup_inputs(case):
    """predict, target, teacher (float32 / int64).  Rows whose fp64 entropy is neither a[lo] nor a[hi] and lies within the
    margin of the threshold are marked ignored and the order statistics derived again, until none is left; the tie
    block is placed afterwards (it moves rows ONTO a value that is already there)."""
    rng = np.random.Generator(np.random.PCG64(case.seed))
    B, K = case.B, case.K
    predict = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32) * 2)
    teacher = torch.from_numpy((rng.standard_normal((B, K)) * rng.uniform(0.2, 4.0, (B, 1))).astype(np.float32))
    target = torch.from_numpy(rng.integers(0, K, B, dtype=np.int64))
    if case.ignored:
        target[torch.from_numpy(rng.choice(B, case.ignored, replace=False))] = O.IGNORE
    for _ in range(50):
        o = unsup_order(teacher, target, case.percent)
        e, a = o["e64"], o["e64"][o["order"]]
        near = (target != O.IGNORE) & ((e - o["thr"]).abs() < o["eps"]) & (e != a[o["lo"]]) & (e != a[o["hi"]])
        if o["g"] > 0 and 0 < float(a[o["hi"]] - a[o["lo"]]) * o["g"] < o["eps"]:
            near[o["order"][o["hi"]]] = True            # a[lo] would sit within the margin below the threshold
        if not bool(near.any()):
            break
        target[near] = O.IGNORE
    if case.variant.startswith("tie"):
        lo, hi, order = o["lo"], o["hi"], o["order"]
        first = {"tie_in": lo - 1, "tie_lo": lo - TIE_ROWS + 1, "tie_above": hi + 2}[case.variant]
        assert first >= 0 and first + TIE_ROWS < o["n"]
        for r in order[first + 1:first + TIE_ROWS]:
            teacher[r] = teacher[order[first]]
    return predict, target, teacher


def unsup_conditions(case, target, teacher):
    """what the inputs of a case must show in fp64, asserted on the CPU; returns a short description"""
    o = unsup_order(teacher, target, case.percent)
    e, a, lo, hi, g, thr, eps = o["e64"], o["e64"][o["order"]], o["lo"], o["hi"], o["g"], o["thr"], o["eps"]
    valid = target != O.IGNORE
    if case.ignored:
        assert int((~valid).sum()) >= case.ignored
    off = valid & (e != a[lo]) & (e != a[hi])
    gap = float((e[off] - thr).abs().min()) if bool(off.any()) else float("inf")
    assert gap >= eps, (case.name, gap, eps)                    # the oracle's dropped set is the only admissible one
    if g > 0 and a[hi] != a[lo]:
        assert float(a[hi] - a[lo]) * g >= eps, case.name      # ... also for the row at a[lo], which stays
    if case.g:
        assert {"zero": g == 0, "low": 0 < g < 0.5, "high": g >= 0.5}[case.g], (case.name, g)
    m = TIE_ROWS
    if case.variant == "tie_in":
        assert a[lo - 1] == a[lo] == a[hi] == a[lo + 2] and a[lo - 2] < a[lo] < a[lo + 3]
    elif case.variant == "tie_lo":
        assert a[lo - m + 1] == a[lo] and a[lo - m] < a[lo] < a[hi]
    elif case.variant == "tie_above":
        assert a[hi] < a[hi + 2] == a[hi + 1 + m] and a[hi + 1] < a[hi + 2] < a[hi + 2 + m]
    elif case.variant in ("n1", "n2"):
        assert o["n"] == int(case.variant[1])
    if case.name.endswith("g0"):
        assert o["n"] == 101
    return f"n {o['n']} lo {lo} g {g:.3f} margin {gap:.1e} (asked {eps:.1e})"


# ============================================================================================ cmlpl_memobank_loss
GENERAL = 0             # MbPlan.kernel: mb_infonce_all_kernel; 1 .. 4: mb_infonce_fast_kernel<NCH>
NL = 120                # labelled rows of every case
I_ITER = 7              # ema = min(1 - 1 / 7, 0.999)
TEMP = 0.5
FEATURES = ("wrapped_ring", "caps_differ", "m_gt_cap", "empty_bank_skipped", "empty_pool", "absent_classes",
            "zero_anchor", "zero_bank_row", "p03", "p1", "rank_tie", "pool3_q256")


class CCase(NamedTuple):
    name: str
    D: int; NN: int; K: int; Q: int; N: int
    mom: str            # "" (no momentum prototype) | "on" | "zero" (given, all zero)
    absent: tuple       # classes without a row: loop position != class
    kernel: int         # the plan under the default switches
    seed: int
    why: str


def _cc(name, D, NN, K, Q, N, mom, kernel, why, absent=(0,)):
    return CCase(name, D, NN, K, Q, N, mom, absent, kernel, 500 + len(name) + D + NN, why)


CCASES = [
    _cc("small", 4, 1, 6, 256, 300, "", 1, "fast<1> at its smallest: one float4 per key, one negative; every class present", absent=()),
    _cc("f1-d4-n50", 4, 50, 6, 256, 301, "on", 1, "fast<1>, one float4 per key, the wrapper's 50 negatives"),
    _cc("f1-d4-n63", 4, 63, 6, 256, 300, "zero", 1, "fast<1>, every key slot of every wave (NK = 64)"),
    _cc("f1-d256-n1", 256, 1, 6, 256, 301, "zero", 1, "fast<1>, full chunk, two keys"),
    _cc("f1-d256-n50", 256, 50, 6, 256, 300, "on", 1, "fast<1>, full chunk: the wrapper's shape"),
    _cc("f1-d256-n63", 256, 63, 6, 256, 301, "", 1, "fast<1> full: 16 keys per wave of 256 floats"),
    _cc("f2-d260", 260, 31, 6, 100, 301, "", 2, "fast<2>, one float4 in the second chunk"),
    _cc("f2-d512", 512, 31, 6, 100, 300, "on", 2, "fast<2>, full second chunk"),
    _cc("f3-d516", 516, 19, 6, 64, 300, "on", 3, "fast<3>, one float4 in the third chunk"),
    _cc("f3-d768", 768, 19, 6, 64, 301, "", 3, "fast<3>, full third chunk"),
    _cc("f4-d772", 772, 15, 6, 64, 301, "zero", 4, "fast<4>, one float4 in the fourth chunk"),
    _cc("f4-d1024", 1024, 15, 6, 64, 300, "on", 4, "fast<4> full: the largest D of the fast kernel"),
    _cc("g-d6", 6, 50, 6, 64, 300, "on", GENERAL, "mb_infonce_all_kernel: D not a multiple of 4, less than a wave of floats"),
    _cc("g-d255", 255, 50, 6, 64, 301, "", GENERAL, "mb_infonce_all_kernel: D = 255"),
    _cc("g-d1028", 1028, 15, 6, 16, 300, "on", GENERAL, "mb_infonce_all_kernel: D > 1024, five strides of the 256-thread loops"),
    _cc("g-n64", 256, 64, 6, 64, 301, "on", GENERAL, "mb_infonce_all_kernel: NK = 65, the first key of the lane + 64 half"),
    _cc("g-n127", 8, 127, 6, 64, 300, "", GENERAL, "mb_infonce_all_kernel: NK = 128 = MB_MAXKEYS, the lane + 64 half full"),
    _cc("g-k65", 8, 15, 65, 16, 301, "zero", GENERAL, "mb_infonce_all_kernel: K > 64 (the fast kernel holds a class per lane)", absent=(0, 9, 33)),
    _cc("k64-q256", 8, 15, 64, 256, 300, "", 1, "fast<1> at K = 64, Q = 256: mb_scatter_all_kernel's slot list takes exactly 64 KiB of LDS", absent=(0, 9, 33)),
    _cc("q1", 32, 50, 6, 1, 300, "on", 1, "one query per position"),
]
CASE_BY_NAME = {c.name: c for c in CCASES}
STAGED = ("small", "f2-d260", "g-n127")     # run again through select -> proto -> enqueue -> infonce per position -> sum
IN_KERNEL = ("f1-d256-n50", "f2-d512", "f3-d516", "f4-d772")    # in-kernel draws: fast against forced general


class CRun(NamedTuple):
    case: CCase
    env: dict
    kernel: int
    why: str

    @property
    def id(self):
        return f"{self.case.name}-" + ("-".join(f"{k[6:]}={v}" for k, v in self.env.items()) or "default")


def _kname(k):
    return "mb_infonce_all_kernel" if k == GENERAL else f"mb_infonce_fast_kernel<{k}>"


CRUNS = []
for _c in CCASES:
    CRUNS.append(CRun(_c, {}, _c.kernel, f"mb_prepare_kernel + {_kname(_c.kernel)} + mb_scatter_all_kernel: {_c.why}"))
    if _c.kernel != GENERAL:
        CRUNS.append(CRun(_c, {"CMLPL_MB_FAST": "0"}, GENERAL,
                          f"mb_infonce_all_kernel forced on the shape of: {_c.why}"))


def memobank_lds(case, kernel):
    """dynamic LDS of the InfoNCE kernel and of the scatter, as the header states them"""
    return (case.D * 4 if kernel == GENERAL else 16 * case.D), 4 * case.K * case.Q


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def contra_inputs(case):
    """Everything one call reads, float32 / int32 on the CPU, built so that the call meets every condition of
    FEATURES that its shape allows (contra_features tells which).  Classes 1 .. 5 carry the special rows:
      2  more new keys than its capacity of 3;      3  a full ring with head 2;
      4  no key and an empty bank (its position is skipped), and an anchor pool of exactly three rows, one of them the
         upper fp32 neighbour of 0.3 (0.3 itself and its lower neighbour stay out);
      5  a row of probabilities all 1.0 (not a key: prob < 1 fails), a row where classes 2 and 5 tie at ranks 2 / 3
         (class 5 is a key by the class-index tie-break), a roomy bank whose oldest row is all zero."""
    rng = np.random.Generator(np.random.PCG64(case.seed))
    D, K, N, Q = case.D, case.K, case.N, case.Q
    present = [c for c in range(K) if c not in case.absent]
    y = rng.choice(present, N)
    y[:NL][:5 * 6] = np.repeat([1, 2, 3, 4, 5], 6)                   # enough labelled rows of every special class
    y[NL:][:5 * 8] = np.repeat([1, 2, 3, 4, 5], 8)                   # ... and unlabelled ones
    low = (rng.random(N) < 0.7).astype(np.float32)
    high = (rng.random(N) < 0.6).astype(np.float32)
    prob = np.zeros((N, K), dtype=np.float32)

    def values():
        """K distinct probabilities in descending order, the largest in (0.32, 0.7)"""
        v = np.concatenate(([rng.uniform(0.32, 0.7)], rng.dirichlet(np.full(K - 1, 0.6))))
        v[1:] *= 1.0 - v[0]
        return np.sort(v)[::-1]

    def craft(n, c, r):
        """row n: class c at rank r of a descending sort"""
        others = rng.permutation([k for k in range(K) if k != c])
        prob[n, np.concatenate((others[:r], [c], others[r:])).astype(np.int64)] = values()

    for n in range(N):      # labelled rows mostly confident in their class, unlabelled ones spread over the ranks
        craft(n, y[n], 0 if (n < NL and rng.random() < 0.8) else int(rng.integers(0, min(K, 9))))
    lab_of = lambda c: [n for n in range(NL) if y[n] == c]
    unl_of = lambda c: [n for n in range(NL, N) if y[n] == c]
    for n in unl_of(2)[:6]:                                           # class 2: six keys into a bank of capacity 3
        craft(n, 2, 4)
        high[n] = 1
    for n in lab_of(4) + unl_of(4):                                   # class 4: no key; three rows in the anchor pool
        high[n] = 0
        low[n] = 0
    p03 = np.float32(0.3)
    rows4 = lab_of(4)[:5] + unl_of(4)[:3]
    for n, v in zip(rows4, (np.nextafter(p03, np.float32(0)), p03, np.nextafter(p03, np.float32(1)), 0.61, 0.55, 0.1, 0.2, 0.05)):
        craft(n, 4, 1)
        prob[n, 4] = v
        low[n] = 1
    u5 = unl_of(5)
    prob[u5[0], :] = 1.0                                              # every probability exactly 1: class 5 has rank 5
    high[u5[0]] = 1
    others = rng.permutation([k for k in range(K) if k not in (2, 5)])       # classes 2 and 5 equal at ranks 2 / 3
    prob[u5[1], np.concatenate((others[:2], [2, 5], others[2:])).astype(np.int64)] = values()
    prob[u5[1], 5] = prob[u5[1], 2]
    high[u5[1]] = 1
    onehot = np.eye(K, dtype=np.float32)
    caps = np.array([5 + (c * 5) % 7 for c in range(K)], dtype=np.int32)
    caps[1:6] = (9, 3, 7, 6, 60)
    stride = int(caps.max())
    rows = np.array([int(rng.integers(1, caps[c] + 1)) for c in range(K)], dtype=np.int32)
    rows[1:6] = (4, 2, 7, 0, 10)
    head = np.array([int(rng.integers(0, caps[c])) if rows[c] == caps[c] else 0 for c in range(K)], dtype=np.int32)
    head[3] = 2
    ring = rng.standard_normal((K, stride, D)).astype(np.float32)     # slots outside a class's rows hold noise too
    ring[5, 0] = 0                                                    # class 5's oldest row
    inp = dict(
        rep=_f32(rng.standard_normal((N, D))), rep_teacher=_f32(rng.standard_normal((N, D)) * 0.7 + 0.1),
        label_l=_f32(onehot[y[:NL]]), label_u=_f32(onehot[y[NL:]]), prob_l=_f32(prob[:NL]), prob_u=_f32(prob[NL:]),
        low_mask=_f32(low), high_mask=_f32(high), caps=torch.from_numpy(caps), stride=stride,
        ring=_f32(ring), state=torch.from_numpy(np.stack((rows, head), axis=1).astype(np.int32)),
        momentum=None, ema=0.0, tie_row=u5[1], ones_row=u5[0], rows4=rows4)
    if case.mom:
        inp["momentum"] = _f32(rng.standard_normal((K, Q, D)) * 0.5) if case.mom == "on" else torch.zeros(K, Q, D)
        inp["ema"] = min(1 - 1 / I_ITER, 0.999)
    # draws: injected per live position from the plan; the first query of the first live position takes the all-zero
    # anchor row (the first row of that position's pool), the first negative of the first query of the position that
    # reads class 5's bank takes the all-zero bank row
    bank = logical_bank(inp)
    plan = O.contra_draw_plan(inp["label_l"], inp["label_u"], inp["prob_l"], inp["prob_u"], inp["low_mask"].view(-1, 1),
                              inp["high_mask"].view(-1, 1), bank, caps.tolist())
    anchor, neg = {}, {}
    for i, pool, r in plan:
        anchor[i] = torch.from_numpy(rng.integers(0, pool, size=(Q,), dtype=np.int64))
        neg[i] = torch.from_numpy(rng.integers(0, r, size=(Q * case.NN,), dtype=np.int64))
    p0 = plan[0][0]
    zero_row = next(n for n in range(N) if y[n] == p0 and low[n] == 1 and prob[n, p0] > p03)
    inp["rep"][zero_row] = 0
    anchor[p0][0] = 0
    valid = [c for c in range(K) if bool(((y == c) & (low == 1)).any())]
    neg[valid.index(5)][0] = 0
    inp.update(plan=plan, anchor_idx=anchor, neg_idx=neg, zero_row=zero_row)
    return inp


def logical_bank(inp):
    """the banks as the reference holds them: per class the rows oldest first"""
    out = []
    for c in range(inp["ring"].shape[0]):
        r, h = (int(v) for v in inp["state"][c])
        idx = (h + torch.arange(r)) % int(inp["caps"][c])
        out.append(inp["ring"][c].index_select(0, idx))
    return out


def run_oracle(case, inp, dtype):
    """O.contra_memobank_loss on copies of the inputs in `dtype` (the selection stays on the float32 values) ->
    (result dict, d loss / d rep)"""
    rep = inp["rep"].to(dtype).clone().requires_grad_(True)
    mom = inp["momentum"]
    res = O.contra_memobank_loss(
        rep, inp["label_l"], inp["label_u"], inp["prob_l"], inp["prob_u"], inp["low_mask"].view(-1, 1),
        inp["high_mask"].view(-1, 1), [b.to(dtype) for b in logical_bank(inp)],
        [int(r) % int(c) for (r, _), c in zip(inp["state"], inp["caps"])], inp["caps"].tolist(),
        inp["rep_teacher"].to(dtype), anchor_idx=inp["anchor_idx"], neg_idx=inp["neg_idx"],
        momentum_prototype=None if mom is None else mom.view(case.K, case.Q, 1, case.D).to(dtype), i_iter=I_ITER,
        queries=case.Q, negatives=case.NN)
    res["loss"].backward()
    return res, (rep.grad if rep.grad is not None else torch.zeros_like(rep))


def contra_features(case, inp, res):
    """which of FEATURES this call's inputs show, from the oracle's bookkeeping"""
    K, caps, st = case.K, inp["caps"].tolist(), inp["state"].tolist()
    valid, m, lists = res["valid_classes"], res["new_keys"], res["lists"]
    live = [i for i, _, _ in inp["plan"]]
    f = set()
    if any(st[c][1] != 0 for c in valid):
        f.add("wrapped_ring")
    if len(set(caps)) > 1:
        f.add("caps_differ")
    if any(m[c] > caps[c] for c in range(K)):
        f.add("m_gt_cap")
    if any(res["memobank"][vc].shape[0] == 0 for vc in valid):
        f.add("empty_bank_skipped")
    if any(len(lists[i][1]) == 0 for i in range(len(valid))):
        f.add("empty_pool")
    if valid != list(range(len(valid))):
        f.add("absent_classes")
    if any(bool((inp["rep"][lists[i][1][inp["anchor_idx"][i]]] == 0).all(dim=1).any()) for i in live):
        f.add("zero_anchor")
    assert bool((inp["rep"][inp["zero_row"]] == 0).all())
    for i in live:
        if bool((res["memobank"][valid[i]][inp["neg_idx"][i]] == 0).all(dim=1).any()):
            f.add("zero_bank_row")
    prob = torch.cat((inp["prob_l"], inp["prob_u"]))
    p03 = np.float32(0.3)
    a, b, c = inp["rows4"][:3]
    pool4 = set(lists[4][1].tolist())
    if (float(prob[a, 4]), float(prob[b, 4]), float(prob[c, 4])) == (float(np.nextafter(p03, np.float32(0))), float(p03), float(np.nextafter(p03, np.float32(1)))) \
            and a not in pool4 and b not in pool4 and c in pool4 and all(n in lists[4][0].tolist() for n in (a, b, c)):
        f.add("p03")
    keys5 = set(lists[5][2].tolist())
    if bool((prob[inp["ones_row"]] == 1).all()) and inp["ones_row"] not in keys5 and float(inp["high_mask"][inp["ones_row"]]) == 1:
        f.add("p1")
    t = inp["tie_row"]
    ranks = O.class_ranks(prob[t:t + 1])[0]
    if float(prob[t, 2]) == float(prob[t, 5]) and (int(ranks[2]), int(ranks[5])) == (2, 3) and t in keys5:
        f.add("rank_tie")
    p4 = valid.index(4) if 4 in valid else -1
    if case.Q == 256 and len(pool4) == 3 and 4 in live:
        f.add("pool3_q256")
    assert p4 >= 0 and p4 not in live, "class 4's bank is empty: its position is skipped"
    return f


STAGED_WHY = ("the reference's stages composed on the host: mb_select_kernel, mb_proto_kernel, mb_enqueue_kernel + "
              "mb_state_kernel, per live position mb_infonce_kernel + mb_scatter_kernel into a caller-zeroed d_drep, "
              "mb_sum_kernel")
PUSH_WHY = "dequeue_and_enqueue of one class with the keys given: mb_push_kernel + mb_push_state_kernel"
KERNELS = ("mb_select_kernel", "mb_proto_kernel", "mb_enqueue_kernel", "mb_state_kernel", "mb_infonce_kernel",
           "mb_scatter_kernel", "mb_sum_kernel", "us_entropy_kernel", "us_rank_kernel", "us_select_kernel", "us_mask_kernel",
           "us_grad_kernel", "mb_prepare_kernel", "mb_infonce_all_kernel", "mb_infonce_fast_kernel<1>",
           "mb_infonce_fast_kernel<2>", "mb_infonce_fast_kernel<3>", "mb_infonce_fast_kernel<4>", "mb_scatter_all_kernel",
           "mb_push_kernel", "mb_push_state_kernel", "us_onewg_kernel", "us_entropy2_kernel", "us_select1_kernel",
           "us_apply_kernel")      # every __global__ function of csrc/memobank.hip (the template four times)


def expected_after(inp, res):
    """what the enqueue must leave, from the oracle's bookkeeping and the ring's definition: state [K][2] = (rows, head),
    keys_log [K][2] = (new keys, rows), and which ring slots hold which logical row"""
    K = inp["ring"].shape[0]
    state, log = [], []
    for c in range(K):
        cap, (rows, head), m = int(inp["caps"][c]), (int(v) for v in inp["state"][c]), res["new_keys"][c]
        total = rows + m
        rows_after = min(total, cap)
        assert rows_after == res["memobank"][c].shape[0]
        state.append((rows_after, (head + max(total - cap, 0)) % cap))
        log.append((m, rows_after))
    return torch.tensor(state, dtype=torch.int32), torch.tensor(log, dtype=torch.int32)
