"""GPU: every regime of the loss block (csrc/loss.hip) against the fp64 oracle, 1 <= K <= 64.

The three exp(f . f^T / T) products of the block run on one of four kernels -- 16 x 32 tiles, 32 x 32 tiles, tall 128 x 32
tiles, the wide kernel in six instantiations -- chosen by plan_loss_phase1 from the local rows, K, the banks' width and
the compute-unit count; the 32-row and the tall kernel each carry a second epilogue for K > 32 (row sums and
E . bank_probs by half-wave shuffles instead of the LDS product); the two feature-gradient GEMMs take their operands
through LDS or load them directly.  Each run of tests/loss_cases.py is there for ONE regime: the library's plan
(cmlpl_debug_loss_plan; held to the same table without a device by tests/test_loss_plan_cpu.py) is asserted first, then
cmlpl_loss_fwd_bwd runs inside cmlpl_timing_begin / _end (one launch each of loss, loss_graph, loss_dfeat) and every
output is held to O.loss_block on .double() copies of the same inputs, gradients from autograd:

  * the nine scalars (each by itself), the four probability blocks, dlogits and dfeat of both networks, both banks'
    probabilities after the write: max |difference| over the tensor's largest reference element (a tensor the oracle has
    exactly zero everywhere must be exactly zero) within max(2e-6, 4 x d32) -- 2e-6 is BOUND of the shape envelope, d32 the
    fp32 oracle's own distance from the fp64 oracle on that run and tensor, computed here and printed next to the device's;
  * the banks' feature rows bit for bit; the mask counts, the positive and the negative pairs exactly.

Before the device is touched the inputs are held to the fp64 oracle (loss_cases.check_conditions): every comparison that
decides something -- largest smoothed probability against adap_mask, every off-diagonal Q0 against pos_thr and neg_thr,
the top-2 gap of the labelled logits `acc` reads -- has a margin of 1e-4, and the decisions are not trivial (masks neither
all 0 nor all 1 for one network, off-diagonal positive pairs, negative pairs).  docs/EXPERIMENTS.md, "Loss-block
envelope", has the figures and the mutations this table was shown to catch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV
from tests.loss_cases import CASES, KERNELS, RUNS, bank_feats_after, bank_ptr, check_conditions, check_plan, make_inputs, oracle, read_plan
from tests.test_gpu_shape_envelope import BOUND, _launch_counts
from tests.test_gpu_wgrad_envelope import _switches

pytestmark = pytest.mark.gpu
SCALARS = ("ctr_s", "total_s", "cls_s", "con_s", "acc", "total_w", "cls_w", "con_w", "ctr_w")
ORDERED = sorted(RUNS, key=lambda r: CASES.index(r.case))        # a case's runs follow each other: its reference is built once


def _rel(got, ref):
    """max |difference| over the reference's largest element; an all-zero reference asks for exact zeros"""
    d, m = float((got.double() - ref).abs().max()), float(ref.abs().max())
    return d / m if m > 0 else (0.0 if d == 0 else float("inf"))


@functools.lru_cache(maxsize=1)
def _reference(case):
    """inputs, the fp64 oracle's tensors, the fp32 oracle's distance from them, the exact counts -- built once per case,
    shared by its runs, never written to"""
    inputs = make_inputs(case)
    lb, ref = oracle(case, inputs, torch.float64)
    cond = check_conditions(case, inputs, lb)
    lb32, ref32 = oracle(case, inputs, torch.float32)
    d32 = {k: _rel(ref32[k], ref[k]) for k in ref}
    counts = [float(lb["mask_w"].sum()), float(lb["mask_s"].sum()), float((lb["Q"] > 0).sum()), float(lb["n_neg"])]
    assert counts[2] == lb["n_pos"] and counts == [float(lb32["mask_w"].sum()), float(lb32["mask_s"].sum()), lb32["n_pos"], lb32["n_neg"]]
    feats = bank_feats_after(case, inputs)
    assert torch.equal(feats[0][:3], lb["bank0_rows"][0][5:8].float()) and torch.equal(feats[1][3:6], lb["bank1_rows"][0][:3].float())
    return inputs, ref, d32, counts, feats, cond


def _device(case, inputs, cnt):
    from cmlpl_amd import _lib
    lib = _lib.load()
    z, f, Y, bf, bp = inputs
    bt, btu, K, Q = case.bt, case.btu, case.K, case.Q
    n = bt + btu
    hp = O.HyperParams()
    cs = _lib.Shape(60, 20, 20, 103, K)
    d = lambda t: t.to(DEV).contiguous()
    logits, feat, labels = d(torch.stack(z)), d(torch.stack(f)), d(Y)
    bank_f, bank_p = [d(t.clone()) for t in bf], [d(t.clone()) for t in bp]
    banks = _lib.Banks()
    for i in range(2):
        banks.d_feats[i] = bank_f[i].data_ptr(); banks.d_probs[i] = bank_p[i].data_ptr(); banks.ptr[i] = bank_ptr(case)[i]
    banks.Q = Q
    chp = _lib.HParams(hp.lr, hp.beta1, hp.beta2, hp.eps, hp.temperature, hp.alpha, hp.noise, hp.dropout,
                       hp.w_contrast, hp.w_mutual, hp.pos_thr, hp.neg_thr)
    scal = torch.full((16,), 7.0, device=DEV)
    dlog, dfe = torch.full((2, n, K), 7.0, device=DEV), torch.full((2, n, 1024), 7.0, device=DEV)
    probs = torch.full((4, btu, K), 7.0, device=DEV)
    ws = torch.empty(lib.cmlpl_workspace_bytes(C.byref(cs), 2, n, Q), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    with _launch_counts(cnt):
        rc = lib.cmlpl_loss_fwd_bwd(C.byref(cs), bt, btu, logits.data_ptr(), feat.data_ptr(), labels.data_ptr(),
                                    C.byref(banks), int(case.smooth), case.adap, C.byref(chp), scal.data_ptr(), dlog.data_ptr(),
                                    dfe.data_ptr(), probs.data_ptr(), ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream().cuda_stream)
    try:
        assert rc <= 0, f"hipError_t {rc}"
        torch.cuda.synchronize()
    except (AssertionError, RuntimeError) as e:       # nothing more is started on a device that has reported an error
        pytest.exit(f"HIP error in the loss block of case {case.name}: {e}", returncode=3)
    assert rc == 0, rc
    s, pr = scal.cpu(), probs.cpu()
    got = {k: s[i:i + 1] for i, k in enumerate(SCALARS)}
    got.update(p_w=pr[0], p_s=pr[1], p_w0=pr[2], p_s0=pr[3], dlogits_s=dlog[0].cpu(), dlogits_w=dlog[1].cpu(),
               dfeat_s=dfe[0].cpu(), dfeat_w=dfe[1].cpu(), bank0_probs=bank_p[0].cpu(), bank1_probs=bank_p[1].cpu())
    return got, [float(v) for v in s[9:13]], [t.cpu() for t in bank_f]


@pytest.mark.parametrize("run", ORDERED, ids=[r.id for r in ORDERED])
def test_loss_block_against_the_fp64_oracle_in_its_regime(run):
    case = run.case
    inputs, ref, d32, counts, feats, cond = _reference(case)
    cnt = {}
    with _switches(run.env):
        plan = read_plan(case.K, case.bt, case.btu, case.Q, case.smooth)
        print(f"[{run.id}] {run.why}: {KERNELS[plan.kernel]} {plan} inputs {cond}")
        check_plan(run, plan)
        got, got_counts, got_feats = _device(case, inputs, cnt)
    assert (cnt["loss"], cnt["loss_graph"], cnt["loss_dfeat"]) == (1, 1, 1) and sum(cnt.values()) == 3, cnt
    assert set(got) == set(ref)
    errs = {k: _rel(got[k], ref[k]) for k in ref}
    bounds = {k: max(BOUND, 4 * d32[k]) for k in ref}
    worst = max(errs, key=lambda k: errs[k] / bounds[k])
    print({k: f"{errs[k]:.2e} (fp32 oracle {d32[k]:.2e})" for k in errs})
    print(f"[{run.id}] worst {worst} {errs[worst]:.2e} fp32 oracle {d32[worst]:.2e} | largest device {max(errs.values()):.2e} largest fp32 oracle {max(d32.values()):.2e}")
    assert got_counts == counts, (got_counts, counts)
    for i in range(2):
        assert torch.equal(got_feats[i], feats[i]), f"bank{i} feature rows"
    bad = {k: (errs[k], bounds[k]) for k in errs if not (np.isfinite(errs[k]) and errs[k] <= bounds[k])}
    assert not bad, bad
