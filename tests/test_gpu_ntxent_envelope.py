"""GPU: every route and edge of csrc/ntxent.hip (cmlpl_ntxent_fwd_bwd) against an fp64 reference, through the C ABI.

Three kernels -- ntx_sim_kernel, then ntx_grad_kernel (vector) or one of three instantiations of ntx_grad_mfma_kernel --
a planner and two switches.  Each case of tests/ntxent_cases.py is there for ONE edge: the library's plan
(cmlpl_debug_ntxent_plan; held to a hand-written table without a device by tests/test_ntxent_plan_cpu.py) is asserted
first, then the call is made on float32 inputs with the gradients and the loss inside sentinel-filled buffers and a
workspace full of 0xFF bytes, and

  * loss and both gradients are held to the fp64 reference in the per-row metric of tests/ntxent_cases.py, within
    max(BOUND, 8 d32) max(1, 0.5 / T) -- d32 the fp32 reference's own error on the same case, printed beside the
    device's;
  * the guards around every output, the bytes behind the workspace and the inputs are as they were.

Before the device is touched the inputs are held to their conditions on the CPU (ntxent_cases.prepared).  Beside the
table: a refused batch returns CMLPL_E_ARG with nothing launched; stale workspace bytes cannot reach a result; two runs
give the same bytes; every route of the same inputs agrees with the others; tools.models.ContrastiveLoss returns what
the C call returns.  docs/EXPERIMENTS.md, "NT-Xent envelope", has the figures and the mutations this table catches."""
import numpy as np
import pytest
import torch

from tests import ntxent_cases as N
from tests.gpu_util import DEV
from tests.test_gpu_memobank_envelope import _finish
from tests.test_gpu_wgrad_envelope import _switches

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD = 3.5                 # around the inputs
TAIL = 4096               # bytes behind the workspace


def _place(t, off):
    """t [B, D] inside a larger device allocation, its first element `off` floats past a 16-byte boundary"""
    n = t.numel()
    buf = torch.full((4 + off + n + 8,), PAD, device=DEV)
    buf[4 + off: 4 + off + n] = t.flatten().to(DEV)
    view = buf[4 + off: 4 + off + n]
    assert view.data_ptr() % 16 == 4 * off
    return buf, view


def _call(ei, ej, T, offs=(0, 0), fill=0xFF, what="", expect=0):
    """one cmlpl_ntxent_fwd_bwd -> (rc, loss / grad_i / grad_j on the host, the raw output buffer, the workspace);
    guards, workspace tail and inputs are checked here"""
    from cmlpl_amd import _lib
    lib = _lib.load()
    B, D = ei.shape
    bi, vi = _place(ei, offs[0])
    bj, vj = _place(ej, offs[1])
    keep = bi.clone(), bj.clone()
    G, n = 2 * D + 64, B * D                                  # guard rows in front of, between and behind the outputs
    out = torch.full((4 * G + 2 * n + 1,), SENTINEL, device=DEV)
    o_i, o_j, o_l = G, 2 * G + n, 3 * G + 2 * n
    need = lib.cmlpl_ntxent_workspace_bytes(B, D)
    assert need >= 4 * (4 * B * B + 2 * B)
    ws = torch.full((need + TAIL,), fill, dtype=torch.uint8, device=DEV)
    p = out.data_ptr()
    torch.cuda.synchronize()
    rc = lib.cmlpl_ntxent_fwd_bwd(vi.data_ptr(), vj.data_ptr(), B, D, float(T), p + 4 * o_l, p + 4 * o_i, p + 4 * o_j,
                                  ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    _finish(rc, what)
    assert rc == expect, rc
    host = out.cpu()
    guard = torch.ones(out.numel(), dtype=torch.bool)
    if rc == 0:
        guard[o_i: o_i + n] = False
        guard[o_j: o_j + n] = False
        guard[o_l] = False
    assert bool((host[guard] == SENTINEL).all()), f"{int((host[guard] != SENTINEL).sum())} words written outside the outputs"
    assert bool((ws[need:] == fill).all()), "bytes behind the workspace written"
    assert torch.equal(bi, keep[0]) and torch.equal(bj, keep[1]), "inputs written"
    got = dict(loss=host[o_l: o_l + 1].clone(), grad_i=host[o_i: o_i + n].view(B, D).clone(),
               grad_j=host[o_j: o_j + n].view(B, D).clone())
    return rc, got, host, ws


def _hold(name, errs, d32, T, factor=1.0):
    bnd = {k: factor * v for k, v in N.bounds(d32, T).items()}
    print(f"NTX-ENVELOPE {name} " + " ".join(f"{k} {errs[k]:.2e} d32 {d32[k]:.2e} bound {bnd[k]:.2e}" for k in errs))
    bad = {k: (errs[k], bnd[k]) for k in errs if not (np.isfinite(errs[k]) and errs[k] <= bnd[k])}
    assert not bad, bad


@pytest.mark.parametrize("case", N.CASES, ids=[c.name for c in N.CASES])
def test_ntxent_against_the_fp64_reference_on_its_route(case):
    (ei, ej), ref, scale, d32 = N.prepared(case.key)
    with _switches(dict(case.env)):
        plan = N.ntxent_plan(case.B, case.D, case.aligned)
        print(f"[{case.name}] {case.why}: plan {plan}")
        assert plan == N.full_plan(case.B, case.D, case.route, case.ncw), plan
        _, got, _, _ = _call(ei, ej, case.T, case.offs, what=case.name)
    _hold(f"{case.name} route {case.route} ncw {case.ncw}", N.errors(got, ref, scale), d32, case.T)


@pytest.mark.parametrize("B,D,why", N.REFUSED, ids=[f"b{B}-d{D}" for B, D, _ in N.REFUSED])
def test_a_batch_no_route_holds_is_refused_before_anything_is_launched(B, D, why):
    """CMLPL_E_ARG; loss, gradients and guards keep their sentinels, the workspace keeps every byte (ntx_sim_kernel would
    have written S), the inputs are as they were"""
    assert N.ntxent_plan(B, D, D % 4 == 0) == N.E_ARG
    ei, ej = N.inputs("a", B, D)
    rc, _, _, ws = _call(ei, ej, 0.5, fill=0x5A, what=f"refused {B} x {D}", expect=N.E_ARG)
    assert rc == N.E_ARG and bool((ws == 0x5A).all())


@pytest.mark.parametrize("name", ["chunks-b97-d260-ncw1", "chunks-b97-d260-ncw4", "stride-b257-d6"])
def test_stale_workspace_bytes_do_not_reach_the_results(name):
    """S, the partial denominators and the norms live in caller memory: a workspace of 0xFF bytes (NaN) and a zeroed one
    give the same output bytes"""
    case = N.CASE_BY_NAME[name]
    (ei, ej), _, _, _ = N.prepared(case.key)
    with _switches(dict(case.env)):
        assert N.ntxent_plan(case.B, case.D, case.aligned)[:2] == (case.route, case.ncw)
        _, _, dirty, _ = _call(ei, ej, case.T, case.offs, fill=0xFF, what=name)
        _, _, clean, _ = _call(ei, ej, case.T, case.offs, fill=0x00, what=name)
    assert torch.equal(dirty.view(torch.int32), clean.view(torch.int32))


@pytest.mark.parametrize("name", ["chunks-b129-d260-ncw1", "chunks-b129-d260-ncw2", "chunks-b129-d260-ncw4", "stride-b513-d6",
                                  "family-c-d68", "family-c-d67"])
def test_two_runs_give_the_same_bytes(name):
    case = N.CASE_BY_NAME[name]
    (ei, ej), _, _, _ = N.prepared(case.key)
    with _switches(dict(case.env)):
        _, _, one, _ = _call(ei, ej, case.T, case.offs, what=name)
        _, _, two, _ = _call(ei, ej, case.T, case.offs, what=name)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))


@pytest.mark.parametrize("B,D", N.ALL_ROUTES, ids=[f"b{B}-d{D}" for B, D in N.ALL_ROUTES])
def test_every_route_of_the_same_inputs_agrees(B, D):
    """the vector kernel and the 64- / 128- / 256-column MFMA slices: pairwise within twice the bound, in the metric of the
    table (no bit equality: the summation orders differ)"""
    (ei, ej), ref, scale, d32 = N.prepared(("a", B, D, 0.5))
    outs = {}
    for env in N.ROUTE_ENVS:
        with _switches(dict(env)):
            route = N.ntxent_plan(B, D, True)[:2]
            _, outs[route], _, _ = _call(ei, ej, 0.5, what=f"{B} x {D} on route {route}")
    assert set(outs) == {(0, 0), (1, 1), (1, 2), (1, 4)}, set(outs)
    routes = sorted(outs)
    for i, a in enumerate(routes):
        for b in routes[i + 1:]:
            other = {k: v.double() for k, v in outs[b].items()}
            _hold(f"routes-b{B}-d{D} {a} against {b}", N.errors(outs[a], other, scale), d32, 0.5, factor=2.0)


@pytest.mark.parametrize("B,D", [(24, 64), (1, 36), (1, 37)])
def test_contrastive_loss_module_returns_what_the_c_call_returns(B, D):
    """tools.models.ContrastiveLoss on contiguous views 4 bytes off a 16-byte boundary (D = 64: the vector kernel although
    D is a multiple of 4) and on B = 1; backward with an upstream factor scales both gradients"""
    from tools.models import ContrastiveLoss
    ei, ej = N.inputs("a", B, D)
    off = 1 if B > 1 else 0
    _, vi = _place(ei, off)
    _, vj = _place(ej, off)
    xi, xj = vi.view(B, D).requires_grad_(True), vj.view(B, D).requires_grad_(True)
    assert xi.is_contiguous() and xi.data_ptr() % 16 == 4 * off
    assert N.ntxent_plan(B, D, D % 4 == 0 and not off)[0] == (N.MFMA if D % 4 == 0 and not off else N.VECTOR)
    loss = ContrastiveLoss(B, device=DEV, temperature=0.5)(xi, xj)
    (loss * 3.0).backward()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error in ContrastiveLoss {B} x {D}: {e}", returncode=3)
    _, got, _, _ = _call(ei, ej, 0.5, (off, off), what=f"module {B} x {D}")
    assert torch.equal(loss.detach().cpu().reshape(1), got["loss"])
    assert torch.equal(xi.grad.cpu(), got["grad_i"] * 3.0) and torch.equal(xj.grad.cpu(), got["grad_j"] * 3.0)
    if B == 1:              # one pair: its only negative is its positive -- loss 0, gradients 0 within the bound
        _, ref, scale, d32 = N.prepared(("a", B, D, 0.5))
        _hold(f"module-b1-d{D}", N.errors(got, ref, scale), d32, 0.5)
