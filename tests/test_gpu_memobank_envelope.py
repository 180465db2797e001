"""GPU: every route of csrc/memobank.hip against the fp64 oracle, through the C ABI.

The entropy-filtered cross entropy (cmlpl_unsup_loss) has three forms -- one workgroup, three launches, five launches --
with a K <= 16 body in the first two; the memory-bank InfoNCE in one pass (cmlpl_memobank_loss) has a general kernel and
four instantiations of a keys-in-registers kernel; five staged functions and the single-class push stand beside them.
Each run of tests/memobank_cases.py is there for ONE regime: the library's plan (cmlpl_debug_unsup_plan /
cmlpl_debug_memobank_plan; held to the same tables without a device by tests/test_memobank_plan_cpu.py) is asserted
first, then the call is made on float32 inputs and every output is held to the oracle on .double() copies of them:

  * loss, gradients, prototypes: max |difference| over the tensor's largest reference element (a tensor the oracle has
    exactly zero everywhere must be exactly zero) within max(2e-6, 4 x d32) -- 2e-6 is BOUND of the shape envelope, d32
    the fp32 oracle's own distance from the fp64 oracle on that run and tensor, computed here and printed next to the
    device's.  The row of d_drep that belongs to the all-zero anchor is a tensor of its own: its gradient is 1e8 times
    the others' (cosine_similarity's 1e-8 clamp) and would hide them;
  * target, lists, counts, d_state, d_keys_log, d_arow exactly; bank rows bit for bit, slots outside a ring's rows
    untouched.

Before the device is touched the inputs are held to their conditions on the CPU (memobank_cases.unsup_conditions: every
entropy that is not a[lo] or a[hi] is 64 fp32-oracle errors away from the threshold, so the oracle's dropped set is the
only admissible one; memobank_cases.contra_features: the wrapped ring, the over-full enqueue, the skipped positions,
the 0.3 / 1.0 boundaries ... are there).  docs/EXPERIMENTS.md, "Memory-bank envelope", has the figures and the mutations
this table was shown to catch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests import memobank_cases as M
from tests.gpu_util import DEV
from tests.test_gpu_shape_envelope import BOUND
from tests.test_gpu_wgrad_envelope import _switches

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


def _rel(got, ref):
    """max |difference| over the reference's largest element; an all-zero reference asks for exact zeros"""
    if ref.numel() == 0:
        return 0.0
    d, m = float((got.double() - ref.double()).abs().max()), float(ref.abs().max())
    return d / m if m > 0 else (0.0 if d == 0 else float("inf"))


def _lib():
    from cmlpl_amd import _lib
    return _lib


def _finish(rc, what):
    """nothing more is started on a device that has reported an error"""
    try:
        assert rc <= 0, f"hipError_t {rc}"
        torch.cuda.synchronize()
    except (AssertionError, RuntimeError) as e:
        pytest.exit(f"HIP error in {what}: {e}", returncode=3)


def _hold(run_id, errs, d32):
    bounds = {k: max(BOUND, 4 * d32[k]) for k in errs}
    worst = max(errs, key=lambda k: errs[k] / bounds[k])
    print({k: f"{errs[k]:.2e} (fp32 oracle {d32[k]:.2e})" for k in errs})
    print(f"[{run_id}] worst {worst} {errs[worst]:.2e} fp32 oracle {d32[worst]:.2e}")
    bad = {k: (errs[k], bounds[k]) for k in errs if not (np.isfinite(errs[k]) and errs[k] <= bounds[k])}
    assert not bad, bad


# ============================================================================================ cmlpl_unsup_loss
def _unsup_device(predict, target, teacher, percent, what):
    lib = _lib().load()
    B, K = predict.shape
    p, t, tg = predict.to(DEV).contiguous(), teacher.to(DEV).contiguous(), target.clone().to(DEV)
    loss, grad = torch.full((1,), SENTINEL, device=DEV), torch.full((B, K), SENTINEL, device=DEV)
    need = lib.cmlpl_unsup_workspace_bytes(B)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    rc = lib.cmlpl_unsup_loss(p.data_ptr(), tg.data_ptr(), t.data_ptr(), B, K, float(percent), loss.data_ptr(),
                              grad.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    _finish(rc, what)
    assert rc == 0, rc
    return loss.cpu(), grad.cpu(), tg.cpu()


@functools.lru_cache(maxsize=1)
def _unsup_reference(case):
    """inputs, the fp64 oracle's target / loss / gradient, the fp32 oracle's distance -- built once per case, shared by
    its runs, never written to.  A case in which nothing is kept has no loss or gradient to compare (None)."""
    predict, target, teacher = M.unsup_inputs(case)
    cond = M.unsup_conditions(case, target, teacher)
    out = {}
    for dt in (torch.float64, torch.float32):
        p = predict.to(dt).clone().requires_grad_(True)
        loss, tgt = O.unsupervised_loss(p, target.clone(), case.percent, teacher.to(dt))
        if bool((tgt != O.IGNORE).any()):
            loss.backward()
            out[dt] = (tgt, dict(loss=loss.detach().reshape(1), grad=p.grad))
        else:
            out[dt] = (tgt, None)
    tgt, ref = out[torch.float64]
    assert torch.equal(tgt, out[torch.float32][0])
    d32 = None if ref is None else {k: _rel(out[torch.float32][1][k], ref[k]) for k in ref}
    return (predict, target, teacher), tgt, ref, d32, cond


_TARGETS = {}     # case -> the first route's target: every later route of the case must return the same bits


@pytest.mark.parametrize("run", M.URUNS, ids=[r.id for r in M.URUNS])
def test_unsup_loss_against_the_fp64_oracle_on_its_route(run):
    case = run.case
    (predict, target, teacher), tgt, ref, d32, cond = _unsup_reference(case)
    with _switches(run.env):
        plan = M.unsup_plan(case.B, case.K)
        print(f"[{run.id}] {run.why}: plan {plan} inputs {cond}")
        assert plan == (run.route, run.regrows), plan
        loss, grad, got_tgt = _unsup_device(predict, target, teacher, case.percent, run.id)
    assert torch.equal(got_tgt, tgt), f"{int((got_tgt != tgt).sum())} rows differ from the oracle's dropped set"
    assert torch.equal(_TARGETS.setdefault(case.name, got_tgt), got_tgt)
    if ref is None:                                  # nothing kept: include/cmlpl.h, cmlpl_unsup_loss
        assert not np.isfinite(float(loss)) and bool((grad == 0).all()) and bool((got_tgt == O.IGNORE).all())
        return
    _hold(run.id, {"loss": _rel(loss, ref["loss"]), "grad": _rel(grad, ref["grad"])}, d32)


@pytest.mark.parametrize("B,K,percent,all_ignored", M.DEGENERATE)
def test_unsup_loss_with_nothing_kept_is_the_same_on_every_route(B, K, percent, all_ignored):
    """percent = 0, or a batch ignored from the start: target all 255, a zero gradient, a loss that is not finite"""
    case = M.UCase("degenerate", B, K, percent, 900 + B, 0, "", "", "")
    predict, target, teacher = M.unsup_inputs(case._replace(percent=50.0))
    if all_ignored:
        target[:] = O.IGNORE
    for env, route, rr in M.unsup_routes(B, K):
        with _switches(env):
            assert M.unsup_plan(B, K) == (route, rr)
            loss, grad, tgt = _unsup_device(predict, target, teacher, percent, f"degenerate {B} x {K} on route {route}")
        assert bool((tgt == O.IGNORE).all()), (route, int((tgt != O.IGNORE).sum()))
        assert bool((grad == 0).all()), route
        assert not np.isfinite(float(loss)), (route, float(loss))


# ============================================================================================ cmlpl_memobank_loss
@functools.lru_cache(maxsize=2)
def _contra_reference(case):
    """inputs, the fp64 oracle's result and gradient, the fp32 oracle's distance per tensor, the features the inputs show
    -- built once per case, shared by its runs, never written to"""
    inp = M.contra_inputs(case)
    res, grad = M.run_oracle(case, inp, torch.float64)
    feats = M.contra_features(case, inp, res)
    res32, grad32 = M.run_oracle(case, inp, torch.float32)
    assert res32["new_keys"] == res["new_keys"] and res32["valid_classes"] == res["valid_classes"]
    ref, ref32 = _contra_tensors(case, inp, res, grad), _contra_tensors(case, inp, res32, grad32)
    d32 = {k: _rel(ref32[k], ref[k]) for k in ref}
    return inp, res, ref, d32, feats


def _contra_tensors(case, inp, res, grad):
    """the tensors held to the tolerance, from an oracle result (or, with the same keys, from the device)"""
    z = inp["zero_row"]
    rest = torch.ones(case.N, dtype=torch.bool)
    rest[z] = False
    valid = res["valid_classes"]
    out = dict(loss=res["loss"].detach().reshape(1), drep=grad[rest], drep_zero_anchor=grad[z], proto=res["proto"][valid])
    if case.mom:
        out["prototype"] = res["prototype"].reshape(case.K, case.Q, case.D)
    return out


def _contra_call(case, inp, injected=True, seed=0, call=0):
    """one cmlpl_memobank_loss on fresh device copies -> (rc, the call's device buffers)"""
    L = _lib()
    lib = L.load()
    K, D, Q, NN, N = case.K, case.D, case.Q, case.NN, case.N
    d = lambda t: t.to(DEV).contiguous()
    b = dict(rep=d(inp["rep"]), rep_teacher=d(inp["rep_teacher"]), prob_l=d(inp["prob_l"]), prob_u=d(inp["prob_u"]),
             label_l=d(inp["label_l"]), label_u=d(inp["label_u"]), low_mask=d(inp["low_mask"]), high_mask=d(inp["high_mask"]),
             bank=d(inp["ring"].clone()), state=d(inp["state"].clone()), caps=d(inp["caps"]),
             lists=torch.full((K, 3, N), -7, dtype=torch.int32, device=DEV),
             counts=torch.full((K, 3), -7, dtype=torch.int32, device=DEV),
             keys_log=torch.full((K, 2), -7, dtype=torch.int32, device=DEV),
             arow=torch.full((K, Q), -7, dtype=torch.int32, device=DEV),
             proto=torch.full((K, D), SENTINEL, device=DEV), lossq=torch.full((K, Q), SENTINEL, device=DEV),
             ganchor=torch.full((K, Q, D), SENTINEL, device=DEV), drep=torch.full((N, D), SENTINEL, device=DEV),
             total=torch.full((1,), SENTINEL, device=DEV))
    c = L.MemobankCall()
    for k in ("rep", "rep_teacher", "prob_l", "prob_u", "label_l", "label_u", "low_mask", "high_mask"):
        setattr(c, "d_" + k, b[k].data_ptr())
    c.N, c.n_labeled, c.K, c.D, c.queries, c.negatives = N, M.NL, K, D, Q, NN
    c.d_bank, c.d_state, c.d_capacity, c.capacity_stride = b["bank"].data_ptr(), b["state"].data_ptr(), b["caps"].data_ptr(), inp["stride"]
    if injected:             # dense [K][..] tables indexed by loop position
        b["anchor"] = torch.zeros(K, Q, dtype=torch.int64)
        b["neg"] = torch.zeros(K, Q * NN, dtype=torch.int64)
        for i, t in inp["anchor_idx"].items():
            b["anchor"][i] = t
        for i, t in inp["neg_idx"].items():
            b["neg"][i] = t
        b["anchor"], b["neg"] = d(b["anchor"]), d(b["neg"])
        c.d_anchor_draw, c.d_neg_draw = b["anchor"].data_ptr(), b["neg"].data_ptr()
    c.seed, c.call = seed, call
    if inp["momentum"] is not None:
        b["momentum"] = d(inp["momentum"])
        b["momentum_on"] = torch.tensor([int(bool((inp["momentum"] != 0).any()))], dtype=torch.int32, device=DEV)
        b["prototype"] = torch.zeros(K, Q, D, device=DEV)
        c.d_momentum, c.d_momentum_on, c.d_prototype = b["momentum"].data_ptr(), b["momentum_on"].data_ptr(), b["prototype"].data_ptr()
        c.ema = inp["ema"]
    c.temperature = M.TEMP
    for k in ("lists", "counts", "proto", "keys_log", "lossq", "ganchor", "arow", "drep", "total"):
        setattr(c, "d_" + k, b[k].data_ptr())
    torch.cuda.synchronize()
    rc = lib.cmlpl_memobank_loss(C.byref(c), torch.cuda.current_stream().cuda_stream)
    _finish(rc, f"cmlpl_memobank_loss of case {case.name}")
    return rc, b


def _check_bookkeeping(case, inp, res, b, arow=True):
    """the integers and the bank of a call (one pass or staged) against the oracle's bookkeeping, exactly"""
    K = case.K
    counts, lists = b["counts"].cpu(), b["lists"].cpu()
    for c in range(K):
        for t in range(3):
            want = res["lists"][c][t].to(torch.int32)
            assert int(counts[c, t]) == want.numel(), (c, t, int(counts[c, t]), want.numel())
            assert torch.equal(lists[c, t, :want.numel()], want), f"list {t} of class {c}"
    state, log = M.expected_after(inp, res)
    assert torch.equal(b["state"].cpu(), state), (b["state"].cpu().tolist(), state.tolist())
    if "keys_log" in b:
        assert torch.equal(b["keys_log"].cpu(), log)
    ring = b["bank"].cpu()
    for c in range(K):
        cap, (rows, head) = int(inp["caps"][c]), (int(v) for v in state[c])
        slots = (head + torch.arange(rows)) % cap
        assert torch.equal(ring[c].index_select(0, slots), res["memobank"][c].float()), f"bank of class {c}"      # copies: bit-exact
        other = torch.ones(inp["stride"], dtype=torch.bool)
        other[slots] = False
        assert torch.equal(ring[c][other], inp["ring"][c][other]), f"slots outside the rows of class {c}"
    if arow:
        want = torch.full((K, case.Q), -1, dtype=torch.int32)
        for i, _, _ in inp["plan"]:
            want[i] = res["lists"][i][1][inp["anchor_idx"][i]].to(torch.int32)
        assert torch.equal(b["arow"].cpu(), want)


def _device_tensors(case, inp, res, b):
    got = dict(res, loss=b["total"].cpu(), proto=b["proto"].cpu())
    if case.mom:
        got["prototype"] = b["prototype"].cpu()
    return _contra_tensors(case, inp, got, b["drep"].cpu())


@pytest.mark.parametrize("run", M.CRUNS, ids=[r.id for r in M.CRUNS])
def test_memobank_loss_against_the_fp64_oracle_in_its_regime(run):
    case = run.case
    inp, res, ref, d32, feats = _contra_reference(case)
    with _switches(run.env):
        plan = M.memobank_plan(case.D, case.K, case.Q, case.NN)
        print(f"[{run.id}] {run.why}: plan {plan} inputs show {sorted(feats)}")
        assert plan == (run.kernel, *M.memobank_lds(case, run.kernel)), plan
        rc, b = _contra_call(case, inp)
    assert rc == 0, rc
    _check_bookkeeping(case, inp, res, b)
    absent = [c for c in range(case.K) if c not in res["valid_classes"]]
    assert bool(torch.isnan(b["proto"].cpu()[absent]).all())          # the mean of an empty selection
    _hold(run.id, {k: _rel(v, ref[k]) for k, v in _device_tensors(case, inp, res, b).items()}, d32)


def test_memobank_loss_refuses_before_it_launches():
    """K * queries > 16384: CMLPL_E_ARG, and the bank, the ring state and every output are as they were"""
    case = M.CASE_BY_NAME["k64-q256"]._replace(name="k65-q256", K=65)
    inp = M.contra_inputs(case)
    assert M.memobank_plan(case.D, case.K, case.Q, case.NN) == M.E_ARG
    rc, b = _contra_call(case, inp)
    assert rc == M.E_ARG, rc
    assert torch.equal(b["bank"].cpu(), inp["ring"]) and torch.equal(b["state"].cpu(), inp["state"])
    for k in ("lists", "counts", "keys_log", "arow"):
        assert bool((b[k] == -7).all()), k
    for k in ("proto", "lossq", "ganchor", "drep", "total"):
        assert bool((b[k] == SENTINEL).all()), k


@pytest.mark.parametrize("name", M.IN_KERNEL)
def test_in_kernel_draws_are_the_same_in_the_fast_and_the_general_kernel(name):
    """both kernels key the same Philox counters: the same seed / call must draw the same anchors (d_arow, exactly) and
    the same negatives (loss and d_drep to the tolerance of the case's injected run)"""
    case = M.CASE_BY_NAME[name]
    inp, res, ref, d32, _ = _contra_reference(case)
    out = {}
    for env in ({}, {"CMLPL_MB_FAST": "0"}):
        with _switches(env):
            assert M.memobank_plan(case.D, case.K, case.Q, case.NN)[0] == (M.GENERAL if env else case.kernel)
            rc, b = _contra_call(case, inp, injected=False, seed=20260, call=77)
        assert rc == 0, rc
        _check_bookkeeping(case, inp, res, b, arow=False)
        out[bool(env)] = b
    fast, gen = out[False], out[True]
    arow = fast["arow"].cpu()
    assert torch.equal(arow, gen["arow"].cpu())
    live = [i for i, _, _ in inp["plan"]]
    for i in range(case.K):
        if i in live:
            pool = set(res["lists"][i][1].tolist())
            assert set(arow[i].tolist()) <= pool and len(set(arow[i].tolist())) > 1
        else:
            assert bool((arow[i] == -1).all())
    a, g = _device_tensors(case, inp, res, fast), _device_tensors(case, inp, res, gen)
    _hold(f"{name}-in-kernel", {k: _rel(a[k], g[k]) for k in ("loss", "drep", "drep_zero_anchor")}, d32)


# ============================================================================================ the staged functions
def _staged(case, inp):
    """select -> proto -> enqueue -> per live position infonce (+ scatter into a caller-zeroed d_drep) -> sum, composed on
    the host as a caller with the reference's control flow would (the counts and ring state are read back)"""
    lib = _lib().load()
    K, D, Q, NN, N = case.K, case.D, case.Q, case.NN, case.N
    st = torch.cuda.current_stream().cuda_stream
    d = lambda t: t.to(DEV).contiguous()
    rep, rept = d(inp["rep"]), d(inp["rep_teacher"])
    prob, label = d(torch.cat((inp["prob_l"], inp["prob_u"]))), d(torch.cat((inp["label_l"], inp["label_u"])))
    low, high = d(inp["low_mask"]), d(inp["high_mask"])
    b = dict(bank=d(inp["ring"].clone()), state=d(inp["state"].clone()), caps=d(inp["caps"]),
             lists=torch.full((K, 3, N), -7, dtype=torch.int32, device=DEV),
             counts=torch.full((K, 3), -7, dtype=torch.int32, device=DEV), proto=torch.full((K, D), SENTINEL, device=DEV),
             drep=torch.zeros(N, D, device=DEV), total=torch.full((1,), SENTINEL, device=DEV))
    p = lambda t: t.data_ptr()
    rc = lib.cmlpl_memobank_select(p(prob), p(label), p(low), p(high), N, M.NL, K, p(b["lists"]), p(b["counts"]), st)
    rc = rc or lib.cmlpl_memobank_proto(p(rept), N, D, K, p(b["lists"]), p(b["counts"]), p(b["proto"]), st)
    rc = rc or lib.cmlpl_memobank_enqueue(p(rept), N, D, K, p(b["lists"]), p(b["counts"]), p(b["bank"]), p(b["state"]),
                                          p(b["caps"]), inp["stride"], st)
    _finish(rc, f"the staged enqueue of case {case.name}")
    assert rc == 0, rc
    cnt, state = b["counts"].cpu(), b["state"].cpu()
    valid = [c for c in range(K) if int(cnt[c, 0]) > 0]
    lossq = torch.zeros(len(valid), Q, device=DEV)
    ganchor = torch.full((Q, D), SENTINEL, device=DEV)
    keep = []
    for i, vc in enumerate(valid):
        pool_rows, rows, head = int(cnt[i, 1]), int(state[vc, 0]), int(state[vc, 1])
        if pool_rows == 0 or rows == 0:
            continue
        a_idx, n_idx = d(inp["anchor_idx"][i]), d(inp["neg_idx"][i])
        keep += [a_idx, n_idx]
        rc = lib.cmlpl_memobank_infonce(p(rep), N, D, p(b["lists"][i, 1]), pool_rows, p(a_idx), p(b["proto"][i]), 0,
                                        p(b["bank"][vc]), int(inp["caps"][vc]), rows, head, p(n_idx), Q, NN, M.TEMP,
                                        1.0 / len(valid), p(lossq[i]), p(ganchor), p(b["drep"]), st)
        _finish(rc, f"the staged InfoNCE of case {case.name}, position {i}")
        assert rc == 0, rc
    rc = lib.cmlpl_memobank_sum(p(lossq), lossq.numel(), p(b["total"]), st)
    _finish(rc, f"the staged sum of case {case.name}")
    assert rc == 0, rc
    return b


@pytest.mark.parametrize("name", M.STAGED)
def test_staged_functions_equal_the_one_pass_call(name):
    case = M.CASE_BY_NAME[name]
    assert not case.mom
    inp, res, ref, d32, feats = _contra_reference(case)
    print(f"[staged-{name}] {M.STAGED_WHY}: {case.why}")
    rc, one = _contra_call(case, inp)
    assert rc == 0, rc
    b = _staged(case, inp)
    for k in ("lists", "counts", "bank", "state"):
        got, want = b[k].cpu(), one[k].cpu()
        if k == "lists":                                  # (entries past a list's count are scratch)
            cnt = one["counts"].cpu()
            for c in range(case.K):
                for t in range(3):
                    assert torch.equal(got[c, t, :int(cnt[c, t])], want[c, t, :int(cnt[c, t])]), (c, t)
        else:
            assert torch.equal(got, want), k
    _check_bookkeeping(case, inp, res, b, arow=False)
    got = _device_tensors(case, inp, res, b)
    _hold(f"staged-{name}", {k: _rel(got[k], ref[k]) for k in got}, d32)


def test_push_of_one_class_is_a_sliding_window():
    print(f"[push] {M.PUSH_WHY}")
    lib = _lib().load()
    rng = np.random.Generator(np.random.PCG64(77))
    cap, D = 12, 6
    ring = torch.full((cap, D), SENTINEL, device=DEV)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    q_ref, p_ref = torch.zeros(0, D), 0
    for m in (3, 0, 5, 7, 40, 1, 13):                     # fills, wraps, and one batch larger than the ring
        keys = torch.from_numpy(rng.standard_normal((m, D)).astype(np.float32))
        q_ref, p_ref, _ = O.memobank_enqueue(keys, q_ref, p_ref, cap)
        kd = keys.to(DEV)
        rc = lib.cmlpl_memobank_push(kd.data_ptr() if m else None, m, D, ring.data_ptr(), state.data_ptr(), cap,
                                     torch.cuda.current_stream().cuda_stream)
        _finish(rc, "cmlpl_memobank_push")
        assert rc == 0, rc
        rows, head = state.cpu().tolist()
        assert rows == q_ref.shape[0]
        assert torch.equal(ring.cpu().index_select(0, (head + torch.arange(rows)) % cap), q_ref)
