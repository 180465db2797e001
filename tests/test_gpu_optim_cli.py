"""GPU: ``train.py`` with a learning-rate schedule, weight decay and gradient clipping, end to end on the synthetic scene
-- the ``optim`` line, ``--save_optim``, exact resume (eager, ``--graph``, ``--windows cube``), the refusal of a file
written under other options, and the flags at their defaults being no flags at all."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--synthetic", "B2", "--synthetic_scene", "--num_unlabel", "700", "--print_per_batches", "3", "--num_epochs", "2",
        "--no_eval"]
OPTIM = ["--lr_schedule", "cosine", "--warmup_steps", "3", "--lr_min", "1e-5", "--weight_decay", "0.05", "--clip_grad", "0.5"]
STEPS = 12                                  # 2 epochs of ceil(700 / 128) = 6 steps
OPTIM_LINE = re.compile(r"^Epoch (\d)/2: optim lr = (\S+) norm = (\S+) max = (\S+) clipped = (\d+)/6 "
                        r"norm1 = (\S+) max1 = (\S+) clipped1 = (\d+)/6$")


def _run(*args, timeout=600):
    return subprocess.run([sys.executable, "train.py", *BASE, *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def _train(d, tag, *extra):
    hist = os.path.join(d, f"hist_{tag}.npy")
    r = _run("--save_loss_hist", hist, *extra)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines(), np.load(hist)


def _untimed(lines):
    return [ln for ln in lines if not ln.startswith(("training:", "after the first epoch:"))]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("optim"))
    out, hist = _train(d, "S", *OPTIM, "--save_optim", os.path.join(d, "S_optim.npy"), "--ckpt_every", "1",
                       "--save_ckpt", os.path.join(d, "ck{epoch}.pt"))
    return dict(dir=d, S=hist, S_out=out, S_optim=np.load(os.path.join(d, "S_optim.npy")))


def test_save_optim_holds_the_schedule_and_the_norms_and_the_line_sums_them_up(runs):
    from cmlpl_amd.optim import LRSchedule, clip_coef_host
    block, hist = runs["S_optim"], runs["S"]
    assert block.shape == (STEPS, 5) and block.dtype == np.float32 and np.isfinite(block).all()
    assert hist.shape == (STEPS, 5) and np.isfinite(hist).all()
    sched = LRSchedule("cosine", 5e-4, STEPS, warmup_steps=3, lr_min=1e-5)
    want = np.array([np.float32(sched.lr_at(t)) for t in range(1, STEPS + 1)], np.float32)
    assert block[:, 0].tobytes() == want.tobytes()                             # the lr column: float32(lr_at(t))
    assert (block[:, 1:3] > 0).all() and (block[:, 3:] <= 1).all() and (block[:, 3:] > 0).all()
    for t in range(STEPS):
        for n in range(2):                                                     # each coefficient: the fp32 chain on its norm
            assert block[t, 3 + n].tobytes() == clip_coef_host(block[t, 1 + n], 0.5).tobytes()
    lines = [ln for ln in runs["S_out"] if "optim" in ln]
    assert len(lines) == 2 and all(OPTIM_LINE.match(ln) for ln in lines), lines
    for e, ln in enumerate(lines):
        m, rows = OPTIM_LINE.match(ln), block[6 * e:6 * e + 6]
        assert m.group(2) == "%.4e" % rows[-1, 0] and m.group(3) == "%.4f" % rows[:, 1].mean()
        assert m.group(4) == "%.4f" % rows[:, 1].max() and int(m.group(5)) == int((rows[:, 3] < 1).sum())
        assert m.group(7) == "%.4f" % rows[:, 2].max() and int(m.group(8)) == int((rows[:, 4] < 1).sum())
    from cmlpl_amd import checkpoint
    ident = checkpoint.load(os.path.join(runs["dir"], "ck2.pt"))["identity"]
    assert ident["weight_decay"] == 0.05 and ident["clip_grad"] == 0.5
    assert ident["lr_schedule"] == dict(kind="cosine", base_lr=5e-4, total_steps=STEPS, warmup_steps=3, lr_min=1e-5)


@pytest.mark.parametrize("mode", [(), ("--graph",), ("--windows", "cube")], ids=["eager", "graph", "cube"])
def test_resume_after_epoch_1_equals_the_straight_run_bit_for_bit(runs, mode):
    d, tag = runs["dir"], "R" + "".join(m.strip("-") for m in mode)
    out, hist = _train(d, tag, *OPTIM, "--save_optim", os.path.join(d, tag + "_optim.npy"), "--save_ckpt",
                       os.path.join(d, tag + "_{epoch}.pt"), "--resume", os.path.join(d, "ck1.pt"), *mode)
    assert hist.tobytes() == runs["S"].tobytes()                              # loss_hist
    assert np.load(os.path.join(d, tag + "_optim.npy")).tobytes() == runs["S_optim"].tobytes()     # the optim block
    assert [ln for ln in out if "optim" in ln] == [ln for ln in runs["S_out"] if "optim" in ln][1:]
    from cmlpl_amd import checkpoint
    a, b = checkpoint.load(os.path.join(d, "ck2.pt")), checkpoint.load(os.path.join(d, tag + "_2.pt"))
    for k in checkpoint.STATE_TENSORS:
        assert torch.equal(a[k], b[k]), k
    assert (a["ptr"], a["adam_t"], a["step_count"]) == (b["ptr"], b["adam_t"], b["step_count"]) and a["adam_t"] == STEPS
    assert torch.equal(a["extra"]["optim_hist"], b["extra"]["optim_hist"])


def test_resume_under_other_options_refuses_and_names_the_field(runs):
    ck = os.path.join(runs["dir"], "ck1.pt")
    flags = list(OPTIM)
    flags[flags.index("--clip_grad") + 1] = "1.0"
    r = _run(*flags, "--resume", ck)
    assert r.returncode != 0 and "clip_grad: file 0.5, here 1.0" in r.stderr, r.stderr[-2000:]
    assert "weight_decay" not in r.stderr and "lr_schedule" not in r.stderr
    r = _run("--resume", ck)                                                   # no option at all: every field is named
    assert r.returncode != 0 and all(f in r.stderr for f in ("clip_grad", "weight_decay", "lr_schedule")), r.stderr[-2000:]


def test_the_flags_at_their_defaults_are_no_flags(runs, tmp_path):
    from cmlpl_amd import checkpoint
    d = str(tmp_path)
    out_a, hist_a = _train(d, "A", "--save_ckpt", os.path.join(d, "A.pt"))
    out_b, hist_b = _train(d, "B", "--save_ckpt", os.path.join(d, "B.pt"), "--lr_schedule", "constant", "--weight_decay", "0",
                           "--clip_grad", "0")
    assert _untimed(out_a) == _untimed(out_b) and not any("optim" in ln for ln in out_a)
    assert hist_a.tobytes() == hist_b.tobytes() and hist_a.tobytes() != runs["S"].tobytes()
    a, b = checkpoint.load(os.path.join(d, "A.pt")), checkpoint.load(os.path.join(d, "B.pt"))
    assert a["identity"] == b["identity"] and not {"clip_grad", "weight_decay", "lr_schedule"} & set(a["identity"])
    for k in checkpoint.STATE_TENSORS:
        assert torch.equal(a[k], b[k]), k
    assert set(a["extra"]) == set(b["extra"]) and "optim_hist" not in a["extra"]
    strip = lambda args: {k: v for k, v in args.items() if k not in ("save_loss_hist", "save_ckpt")}
    assert strip(a["extra"]["args"]) == strip(b["extra"]["args"]) and "clip_grad" not in a["extra"]["args"]
    r = _run("--save_optim", os.path.join(d, "x.npy"))                         # nothing to save without an option
    assert r.returncode != 0 and "--save_optim" in r.stderr
