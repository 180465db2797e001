"""GPU: the EMA teacher (cmlpl_ema_update, TrainEngine(teacher_alpha=), cmlpl_amd.models.WeightEMA_BN, train.py --ema,
predict.py --net ema*).

Everything here is an EQUALITY of bits: the update is three rounded fp32 operations per element with no reduction, so
the kernel, numpy float32 and the reference's tensor expression (tests/golden/ema, held to the formula on the CPU by
tests/test_ema_host.py) give the same bytes; the step is bit-reproducible, so a run with a teacher beside it, a replayed
run and a resumed run are the straight run."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV
from tests.test_ema_host import FLOAT_KEYS, bits, ema_formula, fixtures

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B2 = (103, 11, 11, 103, 9)
W8 = (40, 8, 8, 40, 5)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _same_bits(got, want):
    """bit equality, NaN-aware: a NaN where a NaN is expected is equal whatever its payload"""
    g, w = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    both_nan = np.isnan(g) & np.isnan(w)
    return bool(((bits(g) == bits(w)) | both_nan).all())


# ------------------------------------------------------------------ the op
COUNTS = (1, 3, 4, 5, 255, 256, 257, 1027, 2 * 552329 + 7)
# (src, ema) offsets in floats into an allocation: aligned alike (the 16-byte path, head of 0 .. 3 floats) and not
OFFSETS = ((0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (3, 2), (2, 0))
GUARD = 8
SENT = np.float32(-12345.678)


@pytest.mark.parametrize("alpha", [0.0, 1.0, 0.5, 0.95, 0.999])
def test_op_equals_the_formula_bit_for_bit(alpha):
    from cmlpl_amd import _lib
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(int(alpha * 1000) + 5))
    nmax = max(COUNTS)
    src_all = (rng.choice([-1.0, 1.0], nmax) * 10.0 ** rng.uniform(-6, 3, nmax)).astype(np.float32)
    ema_all = (rng.choice([-1.0, 1.0], nmax) * 10.0 ** rng.uniform(-6, 3, nmax)).astype(np.float32)
    for count in COUNTS:
        src, ema = src_all[:count].copy(), ema_all[:count].copy()
        # NaN and +-inf at known places of both operands (0 * inf = NaN at alpha 0 / 1 included)
        for i, v in ((0, np.nan), (count // 3, np.inf), (count // 2, -np.inf)):
            src[i] = v
        for i, v in ((count - 1, np.nan), (2 * count // 3, np.inf), (count // 5, -np.inf)):
            ema[i] = v
        with np.errstate(invalid="ignore"):
            want = ema_formula(src, ema, alpha)
        for so, eo in OFFSETS:
            bs = np.full(count + so + 2 * GUARD, SENT, np.float32)
            be = np.full(count + eo + 2 * GUARD, SENT, np.float32)
            bs[GUARD + so: GUARD + so + count] = src
            be[GUARD + eo: GUARD + eo + count] = ema
            ds, de = torch.from_numpy(bs).to(DEV), torch.from_numpy(be).to(DEV)
            assert ds.data_ptr() % 16 == 0 and de.data_ptr() % 16 == 0
            rc = lib.cmlpl_ema_update(ds.data_ptr() + 4 * (GUARD + so), de.data_ptr() + 4 * (GUARD + eo), count, alpha,
                                      _stream())
            assert rc == 0, (count, so, eo, rc)
            got, src_after = de.cpu().numpy(), ds.cpu().numpy()
            lo = GUARD + eo
            assert _same_bits(got[lo:lo + count], want), (alpha, count, so, eo)
            # the guard elements in front of and behind the range, and the source, are untouched
            assert (bits(got[:lo]) == bits(SENT)).all() and (bits(got[lo + count:]) == bits(SENT)).all(), (count, so, eo)
            assert _same_bits(src_after, bs), (count, so, eo)
    # NaN / inf went where the arithmetic says (`want` of the last, the largest count)
    assert np.isnan(want[0]) and np.isnan(want[-1])
    if 0.0 < alpha < 1.0:
        assert np.isinf(want[len(want) // 3]) and np.isinf(want[len(want) // 5])


@pytest.mark.parametrize("count,off", [(1, 0), (5, 1), (257, 3), (1027, 2), (2 * 552329 + 7, 0)])
def test_op_in_place_on_one_buffer(count, off):
    """d_src == d_ema: each element is read before it is written"""
    from cmlpl_amd import _lib
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(count))
    x = (rng.standard_normal(count) * 10.0 ** rng.uniform(-6, 3, count)).astype(np.float32)
    buf = np.full(count + off + 2 * GUARD, SENT, np.float32)
    buf[GUARD + off: GUARD + off + count] = x
    d = torch.from_numpy(buf).to(DEV)
    p = d.data_ptr() + 4 * (GUARD + off)
    assert lib.cmlpl_ema_update(p, p, count, 0.95, _stream()) == 0
    got = d.cpu().numpy()
    assert _same_bits(got[GUARD + off: GUARD + off + count], ema_formula(x, x, 0.95))
    assert (bits(got[:GUARD + off]) == bits(SENT)).all() and (bits(got[GUARD + off + count:]) == bits(SENT)).all()


def test_op_empty_range_launches_nothing():
    from cmlpl_amd import _lib
    lib = _lib.load()
    d = torch.full((16,), 3.0, device=DEV)
    assert lib.cmlpl_ema_update(d.data_ptr(), d.data_ptr(), 0, 0.5, _stream()) == 0
    assert lib.cmlpl_ema_update(None, None, 0, 0.5, _stream()) == 0
    assert bool((d == 3.0).all())


# ------------------------------------------------------------------ the drop-in function against the reference's fixture
class _Tiny(torch.nn.Module):
    """the pair of tests/golden/make_golden_ema.py"""

    def __init__(self):
        super().__init__()
        self.l1, self.l2 = torch.nn.Linear(7, 5), torch.nn.Linear(5, 3)
        self.wide = torch.nn.Parameter(torch.zeros(4099))
        self.register_buffer("count", torch.tensor(0, dtype=torch.int64))


def _load(m, z, prefix):
    m.load_state_dict({k: torch.from_numpy(np.asarray(z[f"{prefix}.{k}"])) for k in FLOAT_KEYS + ("count",)})


def test_drop_in_reproduces_every_state_of_the_reference():
    from tools.models import WeightEMA_BN
    for tag, z in fixtures():
        alpha, calls = float(z["alpha"][0]), int(z["calls"][0])
        base, ens = _Tiny().to(DEV), _Tiny().to(DEV)
        _load(ens, z, "ens0")
        ptrs = {k: v.data_ptr() for k, v in ens.state_dict().items()}
        for c in range(1, calls + 1):
            _load(base, z, f"base{c}")
            v0 = ens.wide._version
            out = WeightEMA_BN(base, ens, alpha)
            assert out is ens and ens.wide._version > v0
            sd = ens.state_dict()
            for k in FLOAT_KEYS:
                got, want = sd[k].cpu().numpy(), z[f"ens{c}.{k}"]
                bad = int((bits(got) != bits(want)).sum())
                print(tag, c, k, "elements that differ:", bad, "of", want.size)
                assert bad == 0, (tag, c, k)
            assert int(sd["count"]) == int(z[f"ens{c}.count"]) and sd["count"].dtype == torch.int64
            # Base is read only, and Ensemble's tensors are updated where they lie
            assert all(torch.equal(v.cpu(), torch.from_numpy(np.asarray(z[f"base{c}.{k}"]))) for k, v in base.state_dict().items())
            assert {k: v.data_ptr() for k, v in sd.items()} == ptrs


# ------------------------------------------------------------------ the engine
BT, STEPS = 8, 5
SCHED = [(0, 15 + s) for s in range(STEPS + 1)]        # crosses the smoothing gate (batch_index > queue_batch = 17)


def _splits(shape=B2, steps=STEPS + 1):
    s = O.NetShape(*shape)
    bs = [O.synthetic_batch(s, BT, BT, 500 + i) for i in range(steps)]
    d = lambda k: torch.cat([b[k] for b in bs]).to(DEV).contiguous()
    idx = torch.arange(steps * BT, dtype=torch.int64, device=DEV)
    return d("XPl"), d("Xl"), d("Y"), d("XPu"), d("Xu"), idx, idx.clone()


def _engine(shape=B2, fresh=False, **kw):
    from cmlpl_amd import HyperParams, NetShape, TrainEngine
    eng = TrainEngine(NetShape(*shape), BT, BT, HyperParams(), device=DEV, seed=11, hist_rows=8, **kw)
    if not fresh:
        s = O.NetShape(*shape)
        eng.load_state_dict(0, O.closed_form_params(s, 1))
        eng.load_state_dict(1, O.closed_form_params(s, 2))
    return eng


def _step(eng, sp, k, **kw):
    XPl, Xl, Y, XPu, Xu, li, ui = sp
    eng.step(XPl, Xl, Y, XPu, Xu, SCHED[k][0], SCHED[k][1], lab_idx=li[k * BT:(k + 1) * BT], unl_idx=ui[k * BT:(k + 1) * BT], **kw)


STATE = ("params", "m", "v", "bank_feats", "bank_probs")


def _assert_same_state(a, b, what, rows=STEPS):
    torch.cuda.synchronize()
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    assert torch.equal(a.scalar_hist[:rows], b.scalar_hist[:rows]), what
    assert a.ptr == b.ptr and a.adam_t == b.adam_t and a.step_count == b.step_count
    assert np.array_equal(a.loss_window(rows), b.loss_window(rows))


@pytest.mark.parametrize("method", ["cmlpl", "cps"])
def test_engine_teacher_follows_the_formula_and_leaves_the_step_alone(method):
    sp = _splits()
    alpha = 0.95
    # the run without a teacher: the parameter block after every step
    A = _engine(method=method)
    assert A.teacher is None and A.teacher_params is None
    snaps = [A.params.cpu().numpy().copy()]
    for k in range(STEPS):
        _step(A, sp, k)
        snaps.append(A.params.cpu().numpy().copy())
    assert not np.array_equal(snaps[0], snaps[-1])
    # the same run with one
    Bn = _engine(method=method, teacher_alpha=alpha)
    for k in range(STEPS):
        _step(Bn, sp, k)
    _assert_same_state(A, Bn, "teacher beside the step")
    assert torch.isfinite(Bn.scalar_hist[:STEPS]).all()
    want = snaps[0].copy()                                    # the teacher starts as the parameters in front of step 1
    for k in range(STEPS):
        want = ema_formula(snaps[k + 1], want, alpha)
    got = Bn.teacher_params.cpu().numpy()
    bad = int((bits(got) != bits(want)).sum())
    print(method, "teacher elements that differ from the folded formula:", bad, "of", want.size)
    assert got.shape == (2, Bn.P) and bad == 0                 # the WHOLE block: dead tensors and padding too
    assert not np.array_equal(got, snaps[-1])
    for net in range(2):
        sd = Bn.teacher.state_dict(net)
        assert list(sd) == Bn.state_dict_keys()
        assert all(torch.equal(sd[k2], Bn.view(Bn.teacher_params, net, k2)) for k2 in sd)
    # a step that does not apply its update leaves the teacher where it is
    before = Bn.teacher_params.clone()
    _step(Bn, sp, STEPS, apply_update=False)
    torch.cuda.synchronize()
    assert torch.equal(Bn.teacher_params, before)
    # replayed: one eager step, then the captured step with the update launched behind every replay
    G = _engine(method=method, teacher_alpha=alpha)
    _step(G, sp, 0)
    g = G.capture(*sp, BT, BT, capacity=8)
    g.program([(SCHED[k][0], SCHED[k][1], k * BT, k * BT) for k in range(1, STEPS)])
    for _ in range(1, STEPS):
        g.launch()
    _assert_same_state(A, G, "replayed with a teacher")
    assert torch.equal(G.teacher_params.cpu(), torch.from_numpy(want)), "replayed teacher"
    g.close()


def test_teacher_restarts_from_the_parameters():
    sp = _splits(steps=3)
    eng = _engine(teacher_alpha=0.5)
    _step(eng, sp, 0)
    _step(eng, sp, 1)
    assert not torch.equal(eng.teacher_params, eng.params)
    eng.teacher_reset()
    assert torch.equal(eng.teacher_params, eng.params)
    # load_state_dict: the next step starts the average anew from what was loaded
    p = O.closed_form_params(O.NetShape(*B2), 7)
    eng.load_state_dict(0, p)
    before = eng.params.clone()
    _step(eng, sp, 2)
    want = ema_formula(eng.params.cpu().numpy(), before.cpu().numpy(), 0.5)
    assert (bits(eng.teacher_params.cpu().numpy()) == bits(want)).all()
    plain = _engine()
    with pytest.raises(RuntimeError, match="teacher_alpha"):
        plain.teacher_reset()


# ------------------------------------------------------------------ evaluation
def _scene(rows, cols, Cc, bands, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    cube = torch.from_numpy(rng.standard_normal((rows, cols, Cc)).astype(np.float32)).to(DEV)
    X = torch.from_numpy(rng.standard_normal((rows * cols, bands)).astype(np.float32)).to(DEV)
    pix = torch.from_numpy(rng.permutation(rows * cols)[:203].astype(np.int64)).to(DEV)
    return cube, X, pix


def _modules(shape, sds):
    from cmlpl_amd.models import BaseNet2
    s = O.NetShape(*shape)
    out = []
    for sd in sds:
        m = BaseNet2(num_features=s.bands, dropout=0.8, num_classes=s.K, in_channels=s.C, window=s.H).to(DEV)
        m.load_state_dict(sd)
        out.append(m.eval())
    return tuple(out)


@pytest.mark.parametrize("shape", [B2, W8], ids=["B2", "W8"])
def test_teacher_evaluates_like_modules_loaded_with_it(shape):
    from cmlpl_amd import NetShape
    from cmlpl_amd.evaluate import Evaluator
    from cmlpl_amd.infer import infer_cube, infer_pixels
    sp = _splits(shape, steps=4)
    eng = _engine(shape, teacher_alpha=0.5)
    cube, X, pix = _scene(16, 16, shape[0], shape[3], 9)
    for k in range(2):
        _step(eng, sp, k)
    stu1 = infer_pixels((eng, None), cube, X, pix, spec_rows=pix, want_logits=True)
    lab, log = infer_pixels((eng.teacher, None), cube, X, pix, spec_rows=pix, want_logits=True)
    assert lab.shape == (2, 203) and log.shape == (2, 203, shape[4]) and torch.isfinite(log).all()
    assert eng.teacher._dirty is False and eng.teacher.packed.data_ptr() != eng.packed.data_ptr()
    mods = _modules(shape, [eng.teacher.state_dict(k) for k in range(2)])
    wl, wz = infer_pixels(mods, cube, X, pix, spec_rows=pix, want_logits=True)
    assert torch.equal(lab, wl) and torch.equal(log, wz)
    assert not torch.equal(log, stu1[1])                       # (the teacher is not the student)
    # the student's evaluation is what it was before the teacher's: the two packed blocks are two blocks
    stu2 = infer_pixels((eng, None), cube, X, pix, spec_rows=pix, want_logits=True)
    assert torch.equal(stu1[0], stu2[0]) and torch.equal(stu1[1], stu2[1])
    smods = _modules(shape, [eng.state_dict(k) for k in range(2)])
    sl, sz = infer_pixels(smods, cube, X, pix, spec_rows=pix, want_logits=True)
    assert torch.equal(stu2[0], sl) and torch.equal(stu2[1], sz)
    # one network of the teacher, through infer_cube
    l1, z1 = infer_cube((eng.teacher, 1), cube, X, want_logits=True)
    assert torch.equal(l1[pix], lab[1]) and torch.equal(z1[pix], log[1])
    # two more steps: the next evaluation follows the NEW teacher (the pack is redone because the update marked it)
    for k in range(2, 4):
        _step(eng, sp, k)
    assert eng.teacher._dirty is True
    lab2, log2 = infer_pixels((eng.teacher, None), cube, X, pix, spec_rows=pix, want_logits=True)
    mods2 = _modules(shape, [eng.teacher.state_dict(k) for k in range(2)])
    wl2, wz2 = infer_pixels(mods2, cube, X, pix, spec_rows=pix, want_logits=True)
    assert torch.equal(lab2, wl2) and torch.equal(log2, wz2)
    assert not torch.equal(log2, log)
    # and the Evaluator takes it as it takes an engine
    truth = torch.from_numpy(np.random.Generator(np.random.PCG64(4)).integers(0, shape[4], 203).astype(np.int64)).to(DEV)
    ev = Evaluator(NetShape(*shape), cube, X, truth, pix, spec_rows=pix)
    cm = ev.evaluate((eng.teacher, None)).cpu().numpy()
    for k in range(2):
        want = np.zeros((shape[4], shape[4]), np.int64)
        np.add.at(want, (truth.cpu().numpy(), lab2[k].cpu().numpy()), 1)
        assert np.array_equal(cm[k], want)


# ------------------------------------------------------------------ checkpoints, one process
def test_engine_checkpoint_carries_the_teacher(tmp_path):
    from cmlpl_amd import checkpoint
    sp = _splits(steps=6)
    A = _engine(teacher_alpha=0.95)
    for k in range(6):
        _step(A, sp, k)
    Bn = _engine(teacher_alpha=0.95)
    for k in range(3):
        _step(Bn, sp, k)
    st = Bn.checkpoint_state()
    assert st["identity"]["teacher_alpha"] == 0.95 and torch.equal(st["teacher_params"], Bn.teacher_params.cpu())
    path = str(tmp_path / "t.ckpt")
    checkpoint.save(path, st)
    ck = checkpoint.load(path)
    for net, key in enumerate(("Teacher", "Teacher1")):
        sd = Bn.teacher.state_dict(net)
        assert list(ck[key]) == list(sd) and all(torch.equal(ck[key][k], sd[k].cpu()) for k in sd)
    Cn = _engine(fresh=True, teacher_alpha=0.95)
    Cn.load_checkpoint_state(ck)
    for k in range(3, 6):
        _step(Cn, sp, k)
    torch.cuda.synchronize()
    assert torch.equal(A.teacher_params, Cn.teacher_params) and torch.equal(A.params, Cn.params)
    # the on-device snapshot of --save_best, re-used
    snap = A.checkpoint_state(on_device=True)
    assert snap["teacher_params"].is_cuda and snap["teacher_params"].data_ptr() != A.teacher_params.data_ptr()
    assert torch.equal(snap["Teacher1"]["conv2.bias"], A.teacher.state_dict(1)["conv2.bias"])
    p = snap["teacher_params"].data_ptr()
    assert A.checkpoint_state(on_device=True, into=snap) is snap and snap["teacher_params"].data_ptr() == p
    # another coefficient is another average
    with pytest.raises(ValueError, match="teacher_alpha"):
        _engine(fresh=True, teacher_alpha=0.9).load_checkpoint_state(ck)
    # a state with a teacher into an engine without one: the teacher is left aside
    Dn = _engine(fresh=True)
    Dn.load_checkpoint_state(ck)
    assert Dn.teacher is None and torch.equal(Dn.params.cpu(), ck["params"])
    # a state without one into an engine with one: the teacher starts from the loaded parameters
    plain = Dn.checkpoint_state()
    assert "teacher_params" not in plain and "Teacher" not in plain and "teacher_alpha" not in plain["identity"]
    En = _engine(fresh=True, teacher_alpha=0.95)
    En.load_checkpoint_state(plain)
    torch.cuda.synchronize()
    assert torch.equal(En.teacher_params, En.params) and torch.equal(En.params.cpu(), plain["params"])


# ------------------------------------------------------------------ the command lines
BASE = ["--synthetic", "B2", "--synthetic_scene", "--num_unlabel", "192", "--labeled_batch_size", "32",
        "--unlabeled_batch_size", "32", "--print_per_batches", "3"]
# what a checkpoint of a run WITHOUT --ema holds: the keys of the parent's files, spelt out
PARENT_KEYS = {"params", "m", "v", "bank_feats", "bank_probs", "range_flags", "Base", "Base1", "ptr", "adam_t", "step_count",
               "seed", "identity", "format_version", "extra"}
PARENT_EXTRA = {"epoch", "num_batches", "loss_hist", "eval_epochs", "eval_curve", "eval_cms", "gen_state", "args", "run", "world"}
PARENT_ARGS = {"dataID", "num_label", "save_path_prefix", "labeled_batch_size", "unlabeled_batch_size", "val_batch_size",
               "num_workers", "lr", "num_epochs", "print_per_batches", "num_unlabel", "thr", "alpha", "queue_batch",
               "temperature", "teacher_alpha", "dropout", "noise", "m", "synthetic", "save_loss_hist", "no_eval", "graph",
               "windows", "synthetic_scene", "eval_every", "save_eval", "save_ckpt", "ckpt_every", "resume", "save_best",
               "report_memory"}
PARENT_RUN = {"lr", "num_epochs", "thr", "alpha", "queue_batch", "temperature", "dropout", "noise", "labeled_batch_size",
              "unlabeled_batch_size", "num_unlabel", "shape", "data"}
PARENT_IDENTITY = {"shape", "hp", "bt", "btu", "Q", "source_hash", "abi"}


def _run(script, *args, env=None, timeout=600):
    e = dict(os.environ, **(env or {}))
    return subprocess.run([sys.executable, script, *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=e)


def _py(script, *args):
    r = _run(script, *args)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _train(d, tag, *extra, epochs=4):
    hist = os.path.join(d, f"hist_{tag}.npy")
    out = _py("train.py", *BASE, "--num_epochs", str(epochs), "--save_loss_hist", hist, *extra)
    return out, np.load(hist)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ema"))
    out, hist = _train(d, "S", "--ema", "--no_eval", "--eval_every", "1", "--save_eval", os.path.join(d, "S.npz"),
                       "--ckpt_every", "2", "--save_ckpt", os.path.join(d, "ck{epoch}.pt"))
    plain_out, plain = _train(d, "plain", "--no_eval", "--save_ckpt", os.path.join(d, "plain.pt"))
    return dict(dir=d, S=hist, S_out=out, S_eval=np.load(os.path.join(d, "S.npz")), plain=plain)


@pytest.mark.parametrize("mode", [(), ("--graph",)], ids=["eager", "graph"])
def test_resumed_run_with_a_teacher_equals_the_straight_run(runs, mode):
    from cmlpl_amd import checkpoint
    d, tag = runs["dir"], "R" + "".join(m.strip("-") for m in mode)
    npz = os.path.join(d, tag + ".npz")
    out, hist = _train(d, tag, "--ema", "--no_eval", "--eval_every", "1", "--save_eval", npz, "--save_ckpt",
                       os.path.join(d, tag + "_{epoch}.pt"), "--resume", os.path.join(d, "ck2.pt"), *mode)
    assert hist.shape == (24, 5) and np.isfinite(hist).all()
    assert hist.tobytes() == runs["S"].tobytes()
    assert hist.tobytes() == runs["plain"].tobytes()               # and the teacher has not moved the run beside it
    z, zs = np.load(npz), runs["S_eval"]
    assert set(zs.files) >= {"curve", "epochs", "cm", "curve_ema", "cm_ema"}
    for k in ("curve", "epochs", "cm", "curve_ema", "cm_ema", "epochs_ema"):
        assert z[k].tobytes() == zs[k].tobytes() and z[k].shape == zs[k].shape, k
    assert zs["curve_ema"].shape == (4, 2, 3) and zs["cm_ema"].shape == (4, 2, 9, 9) and zs["curve"].shape == (4, 2, 3)
    ema_lines = lambda lines: [ln for ln in lines if "validation_ema" in ln]
    assert ema_lines(out) == ema_lines(runs["S_out"])[4:] and len(ema_lines(out)) == 4
    a, b = checkpoint.load(os.path.join(d, "ck4.pt")), checkpoint.load(os.path.join(d, tag + "_4.pt"))
    for k in checkpoint.STATE_TENSORS + ("teacher_params",):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["teacher_params"], a["params"])
    for key in ("Teacher", "Teacher1"):
        assert all(torch.equal(a[key][k], b[key][k]) for k in a[key]) and len(a[key]) == 16
    for k in ("eval_curve", "eval_curve_ema", "eval_cms_ema", "gen_state"):
        assert torch.equal(a["extra"][k], b["extra"][k]), k
    assert a["extra"]["eval_epochs_ema"] == b["extra"]["eval_epochs_ema"] == [1, 2, 3, 4]


def test_resume_refuses_a_run_that_differs_in_ema(runs):
    d = runs["dir"]
    r = _run("train.py", *BASE, "--num_epochs", "4", "--no_eval", "--resume", os.path.join(d, "ck2.pt"))
    assert r.returncode != 0 and "differs" in r.stderr and "ema:" in r.stderr
    r = _run("train.py", *BASE, "--num_epochs", "4", "--no_eval", "--ema", "--resume", os.path.join(d, "plain.pt"))
    assert r.returncode != 0 and "differs" in r.stderr and "ema:" in r.stderr


def test_a_checkpoint_without_ema_has_the_parents_keys(runs):
    from cmlpl_amd import checkpoint
    ck = checkpoint.load(os.path.join(runs["dir"], "plain.pt"))
    assert set(ck) == PARENT_KEYS and set(ck["extra"]) == PARENT_EXTRA
    assert set(ck["extra"]["args"]) == PARENT_ARGS and set(ck["extra"]["run"]) == PARENT_RUN
    assert set(ck["identity"]) == PARENT_IDENTITY
    with_t = checkpoint.load(os.path.join(runs["dir"], "ck2.pt"))
    assert set(with_t) == PARENT_KEYS | {"teacher_params", "Teacher", "Teacher1"}
    assert set(with_t["extra"]) == PARENT_EXTRA | {"eval_epochs_ema", "eval_curve_ema", "eval_cms_ema"}
    assert with_t["identity"]["teacher_alpha"] == 0.95 and with_t["extra"]["run"]["ema"] is True


def test_command_lines(runs, tmp_path):
    from cmlpl_amd import checkpoint
    from cmlpl_amd.infer import infer_cube
    from hsi_loader import SyntheticScene
    F = str(tmp_path / "F.pt")
    out = _py("train.py", "--synthetic", "B2", "--num_epochs", "2", "--eval_every", "1", "--ema", "--save_ckpt", F,
              "--num_unlabel", "128", "--labeled_batch_size", "32", "--unlabeled_batch_size", "32", "--print_per_batches", "2")
    val = [ln for ln in out if re.match(r"^Epoch \d+/2: validation", ln)]
    pat = r"^Epoch %d/2: validation%s OA = \d+\.\d\d AA = \d+\.\d\d Kappa = -?\d+\.\d\d$"
    assert len(val) == 8, val
    for e in range(2):
        for j, tag in enumerate(("", "1", "_ema", "_ema1")):       # the two existing lines, then the two teachers'
            assert re.match(pat % (e + 1, tag), val[4 * e + j]), val[4 * e + j]
    oa = [ln for ln in out if ln.startswith(" OA")]
    assert [ln.split("=")[0] for ln in oa] == [" OA", " OA1", " OA_ema", " OA_ema1"], oa
    ck = checkpoint.load(F)
    assert len(ck["Teacher"]) == 16 and len(ck["Teacher1"]) == 16 and not torch.equal(ck["Teacher"]["conv1.weight"], ck["Base"]["conv1.weight"])
    labels = str(tmp_path / "ema0.npy")
    got = _py("predict.py", "--ckpt", F, "--synthetic", "B2", "--net", "ema0", "--out", labels)
    assert [ln for ln in got if ln.startswith(" OA")] == [oa[2]]
    src = SyntheticScene(B2, 64, 64, seed=3).cube_source(torch.device(DEV))
    mod = _modules(B2, [ck["Teacher"]])[0]
    want = infer_cube(mod, src.cube, src.spectra).cpu().numpy()
    pred = np.load(labels)
    assert pred.shape == (64 * 64,) and pred.dtype == np.int64 and np.array_equal(pred, want)
    both = str(tmp_path / "both.npy")
    _py("predict.py", "--ckpt", F, "--synthetic", "B2", "--net", "ema_both", "--out", both)
    assert np.load(both).shape == (2, 64 * 64) and np.array_equal(np.load(both)[0], want)
    # a file without a teacher
    r = _run("predict.py", "--ckpt", os.path.join(runs["dir"], "plain.pt"), "--synthetic", "B2", "--net", "ema0")
    assert r.returncode != 0 and "--ema" in r.stderr and "Teacher" in r.stderr
    # several GPUs: out at once, with one line
    r = _run("train.py", "--synthetic", "B2", "--ema", "--no_eval", env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "--ema runs on one GPU" in r.stderr
