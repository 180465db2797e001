"""GPU: checkpoints (cmlpl_amd/checkpoint.py, TrainEngine.checkpoint_state / load_checkpoint_state, train.py --save_ckpt /
--ckpt_every / --resume / --save_best, predict.py).

A resumed run must be the straight run, BIT FOR BIT: replays and cube-fed steps are pinned bit-identical to eager
split-fed ones and the gradients are bit-reproducible (no float atomics), so any difference between
a run and its resumed twin is a piece of state the checkpoint lost -- there is no tolerance anywhere in this file except
where W ranks are held against one process (tests/_ckpt_dist_child.py, the figures of tests/_dist_gpu_child.py)."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B2 = (103, 11, 11, 103, 9)
BASE = ["--synthetic", "B2", "--synthetic_scene", "--num_unlabel", "700", "--print_per_batches", "4"]


def _py(script, *args, timeout=900):
    r = subprocess.run([sys.executable, script, *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _train(d, tag, *extra, base=BASE, epochs=4):
    hist = os.path.join(d, f"hist_{tag}.npy")
    out = _py("train.py", *base, "--num_epochs", str(epochs), "--save_loss_hist", hist, *extra)
    return out, np.load(hist)


def _result_block(lines):
    """the lines from the first 'Result:' on, without the timing lines: OA / Kappa / producerA / AA of both networks"""
    i = lines.index("Result:")
    return [ln for ln in lines[i:] if not ln.startswith(("inference time ==", "validation check"))]


# ------------------------------------------------------------------ train.py: exact continuation
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ckpt"))
    plain_out, plain = _train(d, "plain")
    out, hist = _train(d, "S", "--eval_every", "1", "--save_eval", os.path.join(d, "S.npz"), "--ckpt_every", "2",
                       "--save_ckpt", os.path.join(d, "ck{epoch}.pt"))
    return dict(dir=d, plain=plain, plain_out=plain_out, S=hist, S_out=out, S_eval=np.load(os.path.join(d, "S.npz")))


def test_saving_does_not_disturb_training(runs):
    assert runs["S"].shape == (24, 5) and np.isfinite(runs["S"]).all()
    assert runs["S"].tobytes() == runs["plain"].tobytes()
    assert sorted(f for f in os.listdir(runs["dir"]) if f.startswith("ck")) == ["ck2.pt", "ck4.pt"]
    assert _result_block(runs["S_out"]) == _result_block(runs["plain_out"])


@pytest.mark.parametrize("mode", [(), ("--graph",), ("--windows", "cube"), ("--windows", "cube", "--graph")],
                         ids=["eager", "graph", "cube", "cube-graph"])
def test_resumed_run_equals_the_straight_run_bit_for_bit(runs, mode):
    d, tag = runs["dir"], "R" + "".join(m.strip("-") for m in mode)
    npz = os.path.join(d, tag + ".npz")
    out, hist = _train(d, tag, "--eval_every", "1", "--save_eval", npz, "--ckpt_every", "2",
                       "--save_ckpt", os.path.join(d, tag + "_{epoch}.pt"), "--resume", os.path.join(d, "ck2.pt"), *mode)
    S = runs["S"]
    diff = np.flatnonzero((hist != S).any(1))
    print("rows of loss_hist that differ:", diff.tolist(), "max |d| =", float(np.abs(hist - S).max()))
    assert hist.tobytes() == S.tobytes()
    z, zs = np.load(npz), runs["S_eval"]
    for k in ("curve", "epochs", "cm"):
        assert z[k].tobytes() == zs[k].tobytes() and z[k].shape == zs[k].shape, k
    assert _result_block(out) == _result_block(runs["S_out"])
    # only the epochs after the file's ran
    ep = [ln for ln in out if re.match(r"^Epoch \d+/\d+:  \d+/\d+ loss_contrast", ln)]
    assert ep and all(ln.startswith(("Epoch 3/4", "Epoch 4/4")) for ln in ep)
    assert [ln for ln in out if ln.startswith("best validation")] == [ln for ln in runs["S_out"] if ln.startswith("best validation")]
    # and the file it leaves is the straight run's
    from cmlpl_amd import checkpoint
    a, b = checkpoint.load(os.path.join(d, "ck4.pt")), checkpoint.load(os.path.join(d, tag + "_4.pt"))
    for k in checkpoint.STATE_TENSORS:
        assert torch.equal(a[k], b[k]), k
    assert (a["ptr"], a["adam_t"], a["step_count"]) == (b["ptr"], b["adam_t"], b["step_count"])
    assert torch.equal(a["extra"]["gen_state"], b["extra"]["gen_state"])


def test_resuming_a_finished_run_only_evaluates(runs):
    d = runs["dir"]
    out, hist = _train(d, "done", "--resume", os.path.join(d, "ck4.pt"))
    assert hist.tobytes() == runs["S"].tobytes()
    assert "training: 0 steps" in "\n".join(out) and not any(ln.startswith("Epoch ") for ln in out)
    assert _result_block(out) == _result_block(runs["S_out"])
    r = subprocess.run([sys.executable, "train.py", *BASE, "--num_epochs", "4", "--no_eval", "--lr", "0.001", "--resume",
                        os.path.join(d, "ck2.pt")], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "lr:" in r.stderr


# ------------------------------------------------------------------ keep-best and predict.py
def test_save_best_keeps_the_best_validated_epoch(runs):
    d = runs["dir"]
    best = os.path.join(d, "B.pt")
    out, hist = _train(d, "best", "--eval_every", "1", "--save_best", best)
    assert hist.tobytes() == runs["plain"].tobytes()
    line = [ln for ln in out if ln.startswith("best validation:")]
    assert len(line) == 1
    epoch = int(re.match(r"best validation: epoch (\d+) OA", line[0]).group(1))
    from cmlpl_amd import checkpoint
    ck = checkpoint.load(best)
    assert ck["extra"]["epoch"] == epoch and ck["step_count"] == 6 * epoch
    labels = os.path.join(d, "best_labels.npy")
    _py("predict.py", "--ckpt", best, "--synthetic", "B2", "--net", "0", "--out", labels)
    from hsi_loader import SyntheticScene
    truth = SyntheticScene(B2, 64, 64, seed=3).Y.numpy()
    pred = np.load(labels)
    assert pred.shape == (64 * 64,) and pred.dtype == np.int64
    cm = runs["S_eval"]["cm"][epoch - 1, 0]                               # (the same run with --save_eval: integer counts)
    print("epoch", epoch, "correct:", int((pred == truth).sum()), "of", truth.size, "matrix trace:", int(np.trace(cm)))
    assert int((pred == truth).sum()) == int(np.trace(cm)) and truth.size == int(cm.sum())
    assert "%.2f" % (100.0 * (pred == truth).sum() / truth.size) == re.search(r"OA = ([\d.]+)$", line[0]).group(1)


def test_predict_reproduces_the_end_of_run_block(runs):
    d = runs["dir"]
    F = os.path.join(d, "ck4.pt")
    labels = os.path.join(d, "F_labels.npy")
    out = _py("predict.py", "--ckpt", F, "--synthetic", "B2", "--net", "both", "--out", labels)
    assert _result_block(out) == _result_block(runs["S_out"])
    assert sum(ln.startswith(" OA") for ln in out) == 2 and sum(ln.startswith("AA") for ln in out) == 2
    both = np.load(labels)
    assert both.shape == (2, 64 * 64) and both.dtype == np.int64
    one = _py("predict.py", "--ckpt", F, "--synthetic", "B2", "--net", "1")
    assert [ln for ln in one if ln.startswith((" OA", "AA"))] == [ln for ln in out if ln.startswith((" OA1", "AA1"))]
    # in-process: the modules of the file and an engine that loaded the file label the scene alike, bit for bit
    from cmlpl_amd import HyperParams, NetShape, TrainEngine, checkpoint
    from cmlpl_amd.infer import infer_cube
    from hsi_loader import SyntheticScene
    src = SyntheticScene(B2, 64, 64, seed=3).cube_source(torch.device(DEV))
    nets = checkpoint.load_networks(F, DEV)
    eng = TrainEngine(NetShape(*B2), 128, 128, HyperParams(num_epochs=4), device=DEV)
    eng.load_checkpoint_state(checkpoint.load(F))
    for k in range(2):
        assert not nets[k].training
        la, za = infer_cube(nets[k], src.cube, src.spectra, want_logits=True)
        lb, zb = infer_cube((eng, k), src.cube, src.spectra, want_logits=True)
        assert torch.equal(la, lb) and torch.equal(za, zb), k
        assert np.array_equal(la.cpu().numpy(), both[k])


def test_predict_on_the_general_path(tmp_path):
    """20 x 20 x 60 windows (the reference's): no fused forward, the windows are cut chunk by chunk"""
    d = str(tmp_path)
    F = os.path.join(d, "P.pt")
    base = ["--synthetic", "P", "--synthetic_scene", "--num_unlabel", "96", "--labeled_batch_size", "32",
            "--unlabeled_batch_size", "32", "--print_per_batches", "3"]
    out, _ = _train(d, "P", "--save_ckpt", F, base=base, epochs=1)
    got = _py("predict.py", "--ckpt", F, "--synthetic", "P", "--net", "both")
    assert _result_block(got) == _result_block(out)
    r = subprocess.run([sys.executable, "predict.py", "--ckpt", F, "--synthetic", "B2"], cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode != 0 and "shape" in r.stderr


# ------------------------------------------------------------------ the engine interface, one process
STEPS, CUT, BT = 6, 3, 16
SCHED = [(0, 15 + s) for s in range(STEPS)]            # crosses the smoothing gate (batch_index > queue_batch = 17)


def _splits():
    s = O.NetShape(*B2)
    bs = [O.synthetic_batch(s, BT, BT, 500 + i) for i in range(STEPS)]
    d = lambda k: torch.cat([b[k] for b in bs]).to(DEV).contiguous()
    idx = torch.arange(STEPS * BT, dtype=torch.int64, device=DEV)
    return d("XPl"), d("Xl"), d("Y"), d("XPu"), d("Xu"), idx, idx.clone()


def _engine(fresh=False):
    from cmlpl_amd import HyperParams, NetShape, TrainEngine
    eng = TrainEngine(NetShape(*B2), BT, BT, HyperParams(), device=DEV, seed=11, hist_rows=8)
    if not fresh:
        s = O.NetShape(*B2)
        eng.load_state_dict(0, O.closed_form_params(s, 1))
        eng.load_state_dict(1, O.closed_form_params(s, 2))
    return eng


def _step(eng, sp, k):
    XPl, Xl, Y, XPu, Xu, li, ui = sp
    eng.step(XPl, Xl, Y, XPu, Xu, SCHED[k][0], SCHED[k][1], lab_idx=li[k * BT:(k + 1) * BT], unl_idx=ui[k * BT:(k + 1) * BT])


def _flag_word(eng, net):
    off = C.c_int64()
    assert eng.lib.cmlpl_packed_flag_offset(C.byref(eng.cshape), C.byref(off)) == 0
    assert 0 < off.value == eng.packed.shape[1] - 16
    return int(eng.packed[net, off.value:off.value + 1].view(torch.int32).item())


def _assert_same(a, c, what):
    torch.cuda.synchronize()
    for name in ("params", "m", "v", "bank_feats", "bank_probs"):
        x, y = getattr(a, name), getattr(c, name)
        same = torch.equal(x, y)
        print(f"{what}: {name} {'equal' if same else 'DIFFERS, max |d| = %.3e' % float((x - y).abs().max())}")
        assert same, (what, name)
    assert a.ptr == c.ptr and a.adam_t == c.adam_t and a.step_count == c.step_count == STEPS
    assert torch.equal(a.scalar_hist[CUT:STEPS], c.scalar_hist[CUT:STEPS]), what
    assert torch.isfinite(c.scalar_hist[CUT:STEPS]).all()
    assert np.array_equal(a.loss_window(STEPS - CUT), c.loss_window(STEPS - CUT))


@pytest.mark.parametrize("mode", ["eager", "graph", "flag"])
def test_engine_state_through_a_file_continues_bit_for_bit(tmp_path, mode):
    from cmlpl_amd import checkpoint
    sp = _splits()
    old = None

    def run(eng, steps):
        nonlocal old
        for k in steps:
            if mode == "flag" and k == 0:
                # |w| >= 7.9 leaves fp16's range at the packing scale: the full pack of step 1 raises network 1's flag
                sd = eng.state_dict(1)
                old = sd["conv1.weight"][3, 5, 1, 1].clone()
                sd["conv1.weight"][3, 5, 1, 1] = 9.0
                eng.load_state_dict(1, sd)
            _step(eng, sp, k)
            if mode == "flag" and k == 0:
                # back to the old value, straight into the parameters: NOT through load_state_dict, whose full pack
                # would clear the flag -- the flag is sticky until one, so the run stays on the three-piece loops
                eng.view(eng.params, 1, "conv1.weight")[3, 5, 1, 1] = old
    A = _engine()
    run(A, range(STEPS))
    B = _engine()
    run(B, range(CUT))
    if mode == "flag":
        assert _flag_word(B, 1) != 0 and _flag_word(B, 0) == 0 and _flag_word(A, 1) != 0
    else:
        assert _flag_word(B, 0) == 0 and _flag_word(B, 1) == 0
    path = str(tmp_path / "b.ckpt")
    st = B.checkpoint_state()
    checkpoint.save(path, st, dict(note=mode))
    ck = checkpoint.load(path)
    assert ck["step_count"] == CUT and ck["adam_t"] == CUT and ck["seed"] == 11 and ck["extra"]["note"] == mode
    assert int(ck["range_flags"][1, 0]) == _flag_word(B, 1)
    for net, key in enumerate(("Base", "Base1")):
        sd = B.state_dict(net)
        assert list(ck[key]) == list(sd) and len(sd) == 16
        assert all(torch.equal(ck[key][k], sd[k].cpu()) for k in sd)
    Cn = _engine(fresh=True)
    Cn.load_checkpoint_state(ck)
    if mode == "graph":
        _step(Cn, sp, CUT)                       # the first step after a load runs eagerly, the capture follows it
        g = Cn.capture(*sp, BT, BT, capacity=8)
        g.program([(SCHED[k][0], SCHED[k][1], k * BT, k * BT) for k in range(CUT + 1, STEPS)])
        with pytest.raises(RuntimeError, match="pending"):
            Cn.checkpoint_state()                # programmed replays pending: refused, as an eager step is
        with pytest.raises(RuntimeError, match="pending"):
            Cn.load_checkpoint_state(ck)
        for _ in range(CUT + 1, STEPS):
            g.launch()
        Cn.checkpoint_state()                    # (all launched: allowed again)
        _assert_same(A, Cn, mode)
        g.close()
    else:
        run(Cn, range(CUT, STEPS))
        _assert_same(A, Cn, mode)
    if mode == "flag":
        assert _flag_word(Cn, 1) != 0
        # the teeth of this case: WITHOUT the saved flag words the resumed engine's full pack finds every weight in
        # range again, network 1 returns to the two-piece loops, and the run is no longer the straight one
        lost = dict(ck)
        lost["range_flags"] = torch.zeros_like(ck["range_flags"])
        Dn = _engine(fresh=True)
        Dn.load_checkpoint_state(lost)
        run(Dn, range(CUT, STEPS))
        torch.cuda.synchronize()
        assert _flag_word(Dn, 1) == 0
        print("without the flag words: params equal =", torch.equal(A.params, Dn.params),
              "max |d| =", float((A.params - Dn.params).abs().max()))
        assert not torch.equal(A.params, Dn.params)


def test_on_device_snapshot_and_refusals(tmp_path):
    from cmlpl_amd import HyperParams, NetShape, TrainEngine, checkpoint
    sp = _splits()
    A = _engine()
    for k in range(2):
        _step(A, sp, k)
    snap = A.checkpoint_state(on_device=True)
    assert snap["params"].is_cuda and snap["params"].data_ptr() != A.params.data_ptr()
    host = A.checkpoint_state()
    _step(A, sp, 2)
    assert torch.equal(snap["params"].cpu(), host["params"]) and not torch.equal(A.params.cpu(), host["params"])
    p = snap["params"].data_ptr()
    again = A.checkpoint_state(on_device=True, into=snap)             # the second snapshot re-uses the buffers
    assert again is snap and snap["params"].data_ptr() == p and snap["step_count"] == 3
    assert torch.equal(snap["params"], A.params) and torch.equal(snap["Base1"]["conv2.bias"], A.state_dict(1)["conv2.bias"])
    checkpoint.save(str(tmp_path / "s.ckpt"), snap)                    # a device snapshot is written like a host one
    assert torch.equal(checkpoint.load(str(tmp_path / "s.ckpt"))["bank_feats"], A.bank_feats.cpu())
    # identity: every differing field is named
    other = TrainEngine(NetShape(*B2), BT, 2 * BT, HyperParams(lr=1e-3, num_epochs=7), device=DEV)
    with pytest.raises(ValueError) as e:
        other.load_checkpoint_state(host)
    assert all(n in str(e.value) for n in ("hp.lr:", "hp.num_epochs:", "btu:")) and "Q:" not in str(e.value)


def test_two_ranks_save_and_resume(tmp_path):
    """two REAL processes sharing the one GPU over gloo (tests/_ckpt_dist_child.py): rank 0 of a W = 2 pair saves after 3
    steps, a fresh pair loads and runs 3 more -- byte for byte the pair that ran 6 straight, on both ranks; one process
    that loads the same file agrees with the ranks to the tolerances of tests/_dist_gpu_child.py"""
    from cmlpl_amd.launch import spawn_ranks
    rc, out = spawn_ranks(2, [sys.executable, os.path.join(ROOT, "tests", "_ckpt_dist_child.py"), str(tmp_path / "w2.ckpt")],
                          timeout=600)
    assert rc == 0, out
    assert "OK checkpoint world=2" in out, out
