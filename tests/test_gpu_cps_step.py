"""GPU: the whole cross-pseudo-supervision step (cmlpl_train_step with the method set: forward -> CPS loss -> backward
-> Adam) against (a) the fixtures the reference's own step text produced and (b) the CPU restatement (tests/cps_util.py)
side by side on the same explicit noise / dropout masks; then the same step three ways, bit for bit.  Tolerances are
those of tests/test_gpu_step.py for the same quantities."""
import numpy as np
import pytest
import torch

from cmlpl_amd import HyperParams, NetShape, TrainEngine
from cmlpl_amd.patches import extract_patches
from oracle import cmlpl_oracle as O
from tests.cps_util import MARGIN_MIN, CpsCase, cps_cases, cps_step
from tests.golden_util import rel_err
from tests.gpu_util import DEV, cuda_batch, hip_relu_gates, relu_mask_audit, report, report_params, to_hp, to_shape

pytestmark = pytest.mark.gpu
LOSS_RTOL = 1e-4
SHAPES = {"B2": (103, 11, 11, 103, 9), "B5": (48, 15, 15, 48, 20), "P": (60, 20, 20, 103, 9)}


def _engine_from(shape, bt, btu, hp, p0, p1):
    eng = TrainEngine(to_shape(shape), bt, btu, to_hp(hp), device=DEV, method="cps")
    eng.load_state_dict(0, p0)
    eng.load_state_dict(1, p1)
    return eng


def _compare_step(tag, eng, st, b, hp, shape, s, fixture=None):
    """one step on the device and in the restatement (with the device's ReLU decisions); returns the restatement's dict"""
    bt, btu = b["XPl"].shape[0], b["XPu"].shape[0]
    n = bt + btu
    cb = cuda_batch(b)
    eng.step(cb["XPl"], cb["Xl"], cb["Y"], cb["XPu"], cb["Xu"], 0, s, noise=cb["noise"], dropmask=cb["dropmask"])
    gates = hip_relu_gates(eng, shape, n)
    ref = cps_step(st, b, hp, relu_gates=gates)
    assert ref["margin"] >= MARGIN_MIN, (tag, s, ref["margin"])        # the argmax of every row is not a matter of rounding
    sc = eng.read_scalars()
    row = eng.loss_row()
    extra = [sc[k] for k in ("total_w", "cls_w", "con_w")]
    print(f"[{tag}] step {s}: hip={row} restatement={ref['hist']} agree={eng.scalars[13].item()} margin={ref['margin']:.3e}")
    assert row[0] == row[3]                                             # trian_CPS.py:254: column 0 repeats the cross loss
    assert rel_err(row, ref["hist"], 1e-7) < LOSS_RTOL, (s, row, ref["hist"])
    assert rel_err(extra, ref["extra"], 1e-7) < LOSS_RTOL, (s, extra, ref["extra"])
    assert [sc["ctr_s"], sc["ctr_w"], sc["n_pos"], sc["n_neg"]] == [0.0] * 4 and sc["n_mask_w"] == sc["n_mask_s"] == btu
    ps = eng.pseudo_labels().cpu()
    assert torch.equal(ps, ref["pseudo"]), (tag, s)                     # exactly
    assert eng.scalars[13].item() == ref["agree"]
    lo, fe = eng.outputs()
    lo_ref = torch.stack(ref["logits"])
    report("logits", lo, lo_ref, 2e-4, 5e-6 * float(lo_ref.abs().max()) + 2e-5)
    relu_mask_audit(eng, ref["taps"], shape, n, ztol=2e-5 + 0.1 * hp.lr * s, ztol_y=2e-5 + 0.25 * hp.lr * s)
    for net in range(2):
        for k in O.LIVE_KEYS:            # feat_spe.* included: reached through the classifier only, no d_dfeat
            gr = ref["grads"][net][k]
            report(f"grad[{net}] {k}", eng.grad(net, k), gr, 5e-4, 5e-5 * max(float(gr.abs().max()), 1e-4))
    if fixture is not None:
        z = fixture
        assert rel_err(row, z["hist"][s], 1e-7) < LOSS_RTOL, (s, row, z["hist"][s])
        assert rel_err(extra, z["extra"][s], 1e-7) < LOSS_RTOL, (s, extra, z["extra"][s])
        assert np.array_equal(ps.numpy(), z["pseudo"][s]) and eng.scalars[13].item() == int(z["agree"][s])
        gtol = 2e-5 if s == 0 else 5e-3      # (later steps carry another host's ReLU-boundary decisions: test_gpu_step.py)
        report("golden logits", lo, z["logits"][s], 2e-4, 5e-6 * float(lo_ref.abs().max()) + gtol)
    return ref


def _after(eng, st, steps, hp):
    for net in range(2):
        sd = eng.state_dict(net)
        for k in O.LIVE_KEYS:
            report_params(f"param[{net}] {k}", sd[k], st.params[net][k], steps, hp.lr)
        for k in ("feat_ss.weight", "feat_ss2.weight", "feat_ss3.bias"):
            assert torch.equal(sd[k].cpu(), st.params[net][k])
    # no memory bank in this method: banks and pointers are their initial bytes
    assert eng.ptr == [0, 0]
    assert not eng.bank_feats.any() and not eng.bank_probs.any()


@pytest.mark.parametrize("name", cps_cases())
def test_cps_step_matches_reference_fixture_and_restatement(name):
    g = CpsCase(name)
    assert g.margin >= MARGIN_MIN                                       # the stored condition, re-asserted
    p0, p1 = g.params()
    eng = _engine_from(g.shape, g.bt, g.btu, g.hp, p0, p1)
    st = O.StepState.create(g.shape, p0, p1, g.bt, g.hp)
    for s in range(g.steps):
        _compare_step(name, eng, st, g.batch(s), g.hp, g.shape, s, fixture=g.z)
    _after(eng, st, g.steps, g.hp)


@pytest.mark.parametrize("name,bt,btu,steps", [("B2", 128, 128, 3), ("B5", 64, 512, 1)])
def test_cps_step_matches_restatement_at_baseline_batches(name, bt, btu, steps):
    shape = O.NetShape(*SHAPES[name])
    hp = O.HyperParams()
    # walk the seeds until every unlabelled row of every step has a clear argmax in the RESTATEMENT (the condition of the
    # fixtures, decided on the CPU before the device is asked anything)
    for seed in range(50, 90):
        p0, p1 = O.closed_form_params(shape, seed), O.closed_form_params(shape, seed + 1)
        probe = O.StepState.create(shape, p0, p1, bt, hp)
        if all(cps_step(probe, O.synthetic_batch(shape, bt, btu, seed * 1000 + s), hp)["margin"] >= MARGIN_MIN
               for s in range(steps)):
            break
    else:
        pytest.fail("no seed with a clear argmax in every row")
    eng = _engine_from(shape, bt, btu, hp, p0, p1)
    st = O.StepState.create(shape, p0, p1, bt, hp)
    for s in range(steps):
        _compare_step(f"{name} {bt}+{btu} seed {seed}", eng, st, O.synthetic_batch(shape, bt, btu, seed * 1000 + s), hp, shape, s)
    _after(eng, st, steps, hp)


# ------------------------------------------------------------------ the same step three ways, bit for bit
def _engine(shape, bt, btu, hist_rows=32, **kw):
    eng = TrainEngine(NetShape(*shape), bt, btu, HyperParams(), device=DEV, seed=1088, hist_rows=hist_rows, **kw)
    eng.init_params_default(1088)
    return eng


def _state(eng):
    return [eng.params.clone(), eng.m.clone(), eng.v.clone(), eng.bank_feats.clone(), eng.bank_probs.clone(),
            eng.scalar_hist.clone(), eng.grads.clone()]


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"{what}: state tensor {i} differs"


def _scene(shape, n_lab, n_unl, seed):
    Cc, H, W, bands, K = shape
    rows, cols = H + 9, W + 7
    g = torch.Generator().manual_seed(seed)
    cube = torch.randn(rows, cols, Cc, generator=g)
    lab_pix = torch.randint(0, rows * cols, (n_lab,), generator=g)
    unl_pix = torch.randint(0, rows * cols, (n_unl,), generator=g)
    X = torch.randn(n_lab, bands, generator=g)
    Y = torch.randint(0, K, (n_lab,), generator=g)
    Xu = torch.randn(n_unl, bands, generator=g)
    return [t.to(DEV).contiguous() for t in (cube, lab_pix, unl_pix, X, Y, Xu)]


@pytest.mark.parametrize("name,bt,btu", [("B2", 24, 40), ("P", 16, 16)])
def test_cps_graph_replay_is_bit_identical_to_eager_over_24_steps(name, bt, btu):
    shape = SHAPES[name]
    cube, lab_pix, unl_pix, X, Y, Xu = _scene(shape, 4 * bt + 5, 4 * btu + 3, 11)
    XP, XPu = extract_patches(cube, lab_pix, shape[1]), extract_patches(cube, unl_pix, shape[1])
    g = torch.Generator().manual_seed(5)
    lab_perm = torch.randperm(X.shape[0], generator=g).to(DEV)
    unl_perm = torch.randperm(Xu.shape[0], generator=g).to(DEV)
    steps = 24
    offs = [(k % 4) * bt for k in range(steps)], [(k % 4) * btu for k in range(steps)]
    ea, eb = _engine(shape, bt, btu, method="cps"), _engine(shape, bt, btu, method="cps")
    for k in range(steps):
        ea.step(XP, X, Y, XPu, Xu, k // 4, k % 4, lab_idx=lab_perm[offs[0][k]:offs[0][k] + bt],
                unl_idx=unl_perm[offs[1][k]:offs[1][k] + btu])
    eb.step(XP, X, Y, XPu, Xu, 0, 0, lab_idx=lab_perm[:bt], unl_idx=unl_perm[:btu])
    graph = eb.capture(XP, X, Y, XPu, Xu, lab_perm, unl_perm, bt, btu, capacity=32)
    graph.program([(k // 4, k % 4, offs[0][k], offs[1][k]) for k in range(1, steps)])
    for _ in range(steps - 1):
        graph.launch()
    torch.cuda.synchronize()
    assert ea.ptr == eb.ptr == [0, 0] and ea.adam_t == eb.adam_t == steps and ea.step_count == eb.step_count
    _same(_state(ea), _state(eb), f"{name} after {steps} steps")
    assert torch.equal(ea.pseudo_labels(), eb.pseudo_labels())
    wa, wb = ea.loss_window(steps), eb.loss_window(steps)
    assert wa.tobytes() == wb.tobytes() and np.isfinite(wa).all() and (wa[:, 0] == wa[:, 3]).all()
    assert not eb.bank_feats.any() and not eb.bank_probs.any()
    graph.close()


@pytest.mark.parametrize("name,bt,btu", [("B2", 24, 40), ("P", 16, 16), ("B5", 16, 48)])
def test_cps_split_fed_cube_fed_index_fed_and_row_fed_are_one_step(name, bt, btu):
    shape = SHAPES[name]
    n_lab, n_unl = 3 * bt, 3 * btu
    cube, lab_pix, unl_pix, X, Y, Xu = _scene(shape, n_lab, n_unl, 7)
    XP, XPu = extract_patches(cube, lab_pix, shape[1]), extract_patches(cube, unl_pix, shape[1])
    g = torch.Generator().manual_seed(3)
    e_idx, e_cube, e_rows = (_engine(shape, bt, btu, method="cps") for _ in range(3))
    steps = 4
    for s in range(steps):
        li = torch.randperm(n_lab, generator=g)[:bt].to(DEV)
        ui = torch.randperm(n_unl, generator=g)[:btu].to(DEV)
        kw = dict(apply_update=s > 0)
        e_idx.step(XP, X, Y, XPu, Xu, 0, s, lab_idx=li, unl_idx=ui, **kw)                                   # split-fed, by index
        e_cube.step(None, X, Y, None, Xu, 0, s, lab_idx=li, unl_idx=ui, cube=cube, lab_pix=lab_pix, unl_pix=unl_pix, **kw)
        e_rows.step(XP[li].contiguous(), X[li].contiguous(), Y[li].contiguous(), XPu[ui].contiguous(),
                    Xu[ui].contiguous(), 0, s, **kw)                                                        # the gathered rows
        for other, what in ((e_cube, "cube-fed"), (e_rows, "row-fed")):
            (la, fa), (lb, fb) = e_idx.outputs(), other.outputs()
            assert torch.equal(la, lb) and torch.equal(fa, fb), f"{name} step {s} {what}: logits / features differ"
            _same(_state(e_idx), _state(other), f"{name} step {s} {what}")
            assert torch.equal(e_idx.pseudo_labels(), other.pseudo_labels())
    assert torch.isfinite(e_idx.scalar_hist[:steps]).all()


def test_cmlpl_is_untouched_by_the_method_argument():
    shape, bt, btu = SHAPES["B2"], 32, 32
    cube, lab_pix, unl_pix, X, Y, Xu = _scene(shape, bt, btu, 2)
    XP, XPu = extract_patches(cube, lab_pix, shape[1]), extract_patches(cube, unl_pix, shape[1])
    ea, eb, ec = _engine(shape, bt, btu), _engine(shape, bt, btu, method="cmlpl"), _engine(shape, bt, btu, method="cps")
    assert ea.method == "cmlpl" and ea.hp.w_mutual == 4.0 and ec.hp.w_mutual == 0.1 and "method" not in ea.identity()
    for s in range(5):
        for e in (ea, eb, ec):
            e.step(XP, X, Y, XPu, Xu, 1, s)
    _same(_state(ea), _state(eb), "default constructor vs method='cmlpl'")
    assert ea.ptr == eb.ptr and ea.ptr != [0, 0] and ea.bank_feats.any()
    assert not torch.equal(ea.params, ec.params)                        # (the other method is another step)
    with pytest.raises(RuntimeError):
        ea.pseudo_labels()
