"""CPU: the learning-rate schedule against torch's, the numpy definitions of the clipped, decayed Adam step
(cmlpl_amd/optim.py) against torch.optim.AdamW + clip_grad_norm_ on fp32 tensors, and the optimiser fields of a
checkpoint's identity record.  No GPU, no library call."""
import math

import numpy as np
import pytest
import torch

from cmlpl_amd import HyperParams, NetShape
from cmlpl_amd.checkpoint import check_identity, identity_differences, make_identity
from cmlpl_amd.optim import (LRSchedule, OptimConfig, adamw_host, clip_coef_host, grad_norm_host, keep_host)


# ------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
def test_warmup_end_points_and_the_first_step_behind_it(kind):
    s = LRSchedule(kind, 5e-4, total_steps=100, warmup_steps=10, lr_min=1e-5)
    assert s.lr_at(1) == 5e-4 * 1 / 10 and s.lr_at(10) == 5e-4 * 10 / 10 == 5e-4
    assert s.lr_at(11) == 5e-4                                         # lr_at(warmup + 1) == base
    assert all(s.lr_at(t) < s.lr_at(t + 1) for t in range(1, 10))
    with pytest.raises(ValueError):
        s.lr_at(0)


@pytest.mark.parametrize("kind", ["linear", "cosine"])
@pytest.mark.parametrize("warmup", [0, 7])
def test_decay_is_monotone_and_stays_above_lr_min(kind, warmup):
    s = LRSchedule(kind, 5e-4, total_steps=200, warmup_steps=warmup, lr_min=2e-5)
    lrs = [s.lr_at(t) for t in range(warmup + 1, 201)]
    assert lrs[0] == 5e-4 and all(a > b for a, b in zip(lrs, lrs[1:])) and lrs[-1] > 2e-5
    assert s.lr_at(201) == s.lr_at(200) == s.lr_at(10 ** 6)           # past the end: the last step's rate
    n = 200 - warmup
    if kind == "linear":
        assert lrs[-1] == 2e-5 + (5e-4 - 2e-5) * (1 - (n - 1) / n)


def test_constant_without_warmup_is_the_base_rate_exactly():
    s = LRSchedule("constant", 5e-4, total_steps=50)
    assert all(s.lr_at(t) == 5e-4 for t in (1, 2, 49, 50, 51)) and s.is_default()
    assert not LRSchedule("constant", 5e-4, 50, warmup_steps=1).is_default()


@pytest.mark.parametrize("warmup,lr_min", [(0, 0.0), (20, 1e-5)])
def test_cosine_is_torchs_cosine_annealing_stepped_alongside(warmup, lr_min):
    total = 1580
    s = LRSchedule("cosine", 5e-4, total, warmup_steps=warmup, lr_min=lr_min)
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=5e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=total - warmup, eta_min=lr_min)
    worst = 0.0
    for t in range(warmup + 1, total + 1):
        want = opt.param_groups[0]["lr"]                               # torch's rate at its (t - 1 - warmup)-th step
        worst = max(worst, abs(s.lr_at(t) - want) / want)
        opt.step()
        sched.step()
    print(f"cosine vs CosineAnnealingLR over {total - warmup} steps: worst relative difference {worst:.3e}")
    assert worst < 1e-9


def test_schedule_arguments_are_checked():
    for bad in (dict(kind="step"), dict(base_lr=0.0), dict(base_lr=float("nan")), dict(lr_min=1.0), dict(lr_min=-1e-9),
                dict(warmup_steps=-1), dict(total_steps=5, warmup_steps=5)):
        kw = dict(kind="cosine", base_lr=5e-4, total_steps=10)
        kw.update(bad)
        with pytest.raises(ValueError):
            LRSchedule(**kw)
    for bad in (dict(weight_decay=-1.0), dict(clip_grad=float("nan")), dict(clip_grad=float("inf"))):
        with pytest.raises(ValueError):
            OptimConfig(**bad)
    assert not OptimConfig().active() and OptimConfig(clip_grad=1.0).active() and OptimConfig(weight_decay=0.1).active()
    assert OptimConfig(schedule=LRSchedule("constant", 5e-4, 10)).active()


# ------------------------------------------------------------------ the definitions against torch
def test_clip_coefficient_follows_torch():
    f = np.float32
    assert clip_coef_host(f(0.0), 1.0) == f(1.0)                       # 1 / 1e-6 clamped
    assert clip_coef_host(f(100.0), 1.0).tobytes() == (f(1.0) / (f(100.0) + f(1e-6))).tobytes()
    assert clip_coef_host(f(0.5), 1.0) == f(1.0)
    assert np.isnan(clip_coef_host(f("nan"), 1.0))                     # torch's clamp keeps the NaN
    assert clip_coef_host(f("inf"), 1.0) == f(0.0)
    assert clip_coef_host(f("nan"), 0.0) == f(1.0) and clip_coef_host(f(1e30), 0.0) == f(1.0)    # max_norm 0: no clipping
    t = torch.clamp(torch.tensor(1.0) / (torch.tensor(float("nan")) + 1e-6), max=1.0)
    assert torch.isnan(t)


def test_grad_norm_host_walks_the_live_tensors_only():
    off, numel = [0, 8, 12] + [16] * 7 + [16], [7, 3, 4] + [0] * 7 + [100]
    g = np.full(120, 1e30, np.float32)                                 # pads and the dead tensor: poisoned
    g[0:7], g[8:11], g[12:16] = 1.0, 2.0, 3.0
    g[7] = g[11] = np.nan
    S, norm = grad_norm_host(g, off, numel)
    assert S == 7.0 + 12.0 + 36.0 and norm == np.float32(math.sqrt(55.0))
    big = np.zeros(120, np.float32)
    big[0], big[1] = 1e25, 1e-30                                       # squares that fp32 could not hold
    S, norm = grad_norm_host(big, off, numel)
    assert S == float(np.float32(1e25)) ** 2 + float(np.float32(1e-30)) ** 2 and np.isfinite(norm) and norm > 9e24


def test_host_definitions_match_torch_adamw_with_clipping():
    """5 steps, decay 0.05, max_norm 1, gradients of norm ~100: adamw_host + clip_coef_host + grad_norm_host against
    torch.optim.AdamW(foreach=False) + clip_grad_norm_ on CPU fp32 tensors, at the tolerance the project holds its Adam
    to (rtol 1e-6 / atol 1e-7, tests/test_gpu_ops.py)."""
    hp = HyperParams()
    wd, max_norm = 0.05, 1.0
    sizes = [640, 64, 2304, 7, 3]                                       # "tensors" of one network, walked by offset
    off = np.concatenate([[0], np.cumsum([(s + 3) // 4 * 4 for s in sizes])[:-1]]).tolist() + [0] * 5
    numel = sizes + [0] * 5
    total = off[4] + 4
    g0 = torch.Generator().manual_seed(8)
    p = (torch.randn(total, generator=g0) * 0.05).numpy()
    tp = [torch.nn.Parameter(torch.from_numpy(p[o:o + n].copy())) for o, n in zip(off[:5], sizes)]
    opt = torch.optim.AdamW(tp, lr=hp.lr, betas=(hp.beta1, hp.beta2), eps=hp.eps, weight_decay=wd, foreach=False)
    m, v = np.zeros(total, np.float32), np.zeros(total, np.float32)
    worst = 0.0
    for t in range(1, 6):
        g = (torch.randn(total, generator=g0) * (100.0 / math.sqrt(sum(sizes)))).numpy()
        for o, n, q in zip(off[:5], sizes, tp):
            q.grad = torch.from_numpy(g[o:o + n].copy())
        tn = torch.nn.utils.clip_grad_norm_(tp, max_norm, foreach=False)
        opt.step()
        S, norm = grad_norm_host(g, off, numel)
        assert 50 < norm < 200 and abs(float(norm) - float(tn)) <= 2e-6 * float(tn)      # (torch's norm is an fp32 chain)
        coef = clip_coef_host(norm, max_norm)
        for o, n, q in zip(off[:5], sizes, tp):
            s = slice(o, o + n)
            p[s], m[s], v[s] = adamw_host(p[s], g[s], m[s], v[s], t, hp.lr, hp.beta1, hp.beta2, hp.eps, weight_decay=wd,
                                          coef=coef)
            want = q.detach().numpy()
            worst = max(worst, float(np.max(np.abs(p[s] - want) / np.maximum(np.abs(want), 1e-30))))
            np.testing.assert_allclose(p[s], want, rtol=1e-6, atol=1e-7)
            st = opt.state[q]
            np.testing.assert_allclose(m[s], st["exp_avg"].numpy(), rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(v[s], st["exp_avg_sq"].numpy(), rtol=1e-6, atol=1e-7)
    print(f"adamw_host vs torch.optim.AdamW over 5 steps: worst relative difference {worst:.3e}")
    assert keep_host(hp.lr, wd) < 1.0 and keep_host(hp.lr, 0.0) == np.float32(1.0)


def test_everything_off_is_plain_adam_bit_for_bit():
    rng = np.random.default_rng(0)
    p, g = rng.standard_normal(500).astype(np.float32), rng.standard_normal(500).astype(np.float32)
    m, v = np.zeros(500, np.float32), np.zeros(500, np.float32)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=5e-4, foreach=False)
    tp.grad = torch.from_numpy(g.copy())
    opt.step()
    p1, _, _ = adamw_host(p, g, m, v, 1, 5e-4)
    np.testing.assert_allclose(p1, tp.detach().numpy(), rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------ the checkpoint's identity record
def _ident(optim=None):
    return make_identity(NetShape(), HyperParams(), 128, 128, 1280, "0123456789abcdef", 6, optim=optim)


def test_defaults_add_no_key_to_the_identity_record():
    base = make_identity(NetShape(), HyperParams(), 128, 128, 1280, "0123456789abcdef", 6)
    assert _ident(None) == base and _ident(OptimConfig()) == base
    assert _ident(OptimConfig(schedule=LRSchedule("constant", 5e-4, 100))) == base
    assert list(_ident(OptimConfig()).keys()) == list(base.keys())


def test_a_non_default_option_adds_its_key():
    base = _ident()
    assert set(_ident(OptimConfig(weight_decay=0.05))) - set(base) == {"weight_decay"}
    assert set(_ident(OptimConfig(clip_grad=1.0))) - set(base) == {"clip_grad"}
    rec = _ident(OptimConfig(schedule=LRSchedule("cosine", 5e-4, 1580, warmup_steps=20, lr_min=1e-5)))
    assert set(rec) - set(base) == {"lr_schedule"}
    assert rec["lr_schedule"] == dict(kind="cosine", base_lr=5e-4, total_steps=1580, warmup_steps=20, lr_min=1e-5)
    full = _ident(OptimConfig(LRSchedule("linear", 5e-4, 10), 0.05, 1.0))
    assert set(full) - set(base) == {"weight_decay", "clip_grad", "lr_schedule"}
    import io
    buf = io.BytesIO()
    torch.save(full, buf)                                              # plain values: loads with weights_only
    buf.seek(0)
    assert torch.load(buf, weights_only=True) == full


def test_a_mismatch_is_reported_by_field_name():
    a = _ident(OptimConfig(LRSchedule("cosine", 5e-4, 1580, 20), 0.05, 1.0))
    check_identity(a, _ident(OptimConfig(LRSchedule("cosine", 5e-4, 1580, 20), 0.05, 1.0)))
    d = identity_differences(a, _ident(OptimConfig(LRSchedule("cosine", 5e-4, 1580, 20), 0.05, 2.0)))
    assert d == ["clip_grad: file 1.0, here 2.0"]
    d = identity_differences(a, _ident(OptimConfig(LRSchedule("cosine", 5e-4, 790, 20), 0.05, 1.0)))
    assert d == ["lr_schedule.total_steps: file 1580, here 790"]
    d = identity_differences(a, _ident())
    assert sorted(x.split(":")[0] for x in d) == ["clip_grad", "lr_schedule", "weight_decay"]
    d = identity_differences(_ident(), _ident(OptimConfig(weight_decay=0.01)))
    assert d == ["weight_decay: file 0.0, here 0.01"]
    with pytest.raises(ValueError, match="clip_grad"):
        check_identity(a, _ident(OptimConfig(LRSchedule("cosine", 5e-4, 1580, 20), 0.05, 0.0)))
