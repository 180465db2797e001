"""Learning-rate schedules, decoupled weight decay and gradient-norm clipping (host side).

The reference trains with ``torch.optim.Adam`` at one fixed ``--lr`` (train.py:131-132).  This module holds what the
build adds around that step -- ``LRSchedule`` (warm-up, then constant / linear / cosine decay), ``OptimConfig`` (the
options of a ``TrainEngine``) -- and the DEFINITIONS of the device side in numpy (``grad_norm_host``, ``clip_coef_host``,
``adamw_host``: include/cmlpl.h, "THE DEFINITION OF A CLIPPED, DECAYED ADAM STEP"), which the tests hold the kernels to.
Nothing here touches a GPU.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

KINDS = ("constant", "linear", "cosine")
NUM_LIVE = 10         # the live tensors of a network come first in its flat block (cmlpl_layout_t)
OPTIM_COLUMNS = ("lr", "norm", "norm1", "coef", "coef1")      # train.py --save_optim: one row per step


class LRSchedule:
    """The learning rate of the 1-based Adam step ``t``, in Python double.

    ``t <= warmup_steps``: ``base_lr * t / warmup_steps`` (linear warm-up; its last step has the full rate).  Afterwards,
    with ``s = t - 1 - warmup_steps`` and ``n = total_steps - warmup_steps``:
      constant  ``base_lr``
      linear    ``lr_min + (base_lr - lr_min) * (1 - s / n)``
      cosine    ``lr_min + (base_lr - lr_min) * 0.5 * (1 + cos(pi * s / n))`` -- torch's
                ``CosineAnnealingLR(T_max=n, eta_min=lr_min)`` at its ``s``-th step
    so ``lr_at(warmup_steps + 1) == base_lr``, and the decay would reach ``lr_min`` one step behind the last.  Steps past
    ``total_steps`` stay at the last step's rate.
    """

    def __init__(self, kind: str, base_lr: float, total_steps: int, warmup_steps: int = 0, lr_min: float = 0.0):
        if kind not in KINDS:
            raise ValueError(f"lr schedule {kind!r}: one of {', '.join(KINDS)}")
        self.kind, self.base_lr, self.lr_min = kind, float(base_lr), float(lr_min)
        self.total_steps, self.warmup_steps = int(total_steps), int(warmup_steps)
        if not (self.base_lr > 0.0 and math.isfinite(self.base_lr)):
            raise ValueError(f"base_lr {base_lr!r}: a positive rate")
        if not 0.0 <= self.lr_min <= self.base_lr:
            raise ValueError(f"lr_min {lr_min!r}: in [0, base_lr]")
        if self.warmup_steps < 0:
            raise ValueError(f"warmup_steps {warmup_steps!r}: not negative")
        if self.total_steps <= self.warmup_steps:
            raise ValueError(f"total_steps {total_steps!r}: more than the {self.warmup_steps} warm-up steps")

    def lr_at(self, t: int) -> float:
        t = int(t)
        if t < 1:
            raise ValueError(f"Adam steps count from 1, got {t}")
        if t <= self.warmup_steps:
            return self.base_lr * t / self.warmup_steps
        if self.kind == "constant":
            return self.base_lr
        n = self.total_steps - self.warmup_steps
        s = min(t, self.total_steps) - 1 - self.warmup_steps
        if self.kind == "linear":
            return self.lr_min + (self.base_lr - self.lr_min) * (1.0 - s / n)
        return self.lr_min + (self.base_lr - self.lr_min) * 0.5 * (1.0 + math.cos(math.pi * s / n))

    def record(self) -> Dict[str, Any]:
        return dict(kind=self.kind, base_lr=self.base_lr, total_steps=self.total_steps,
                    warmup_steps=self.warmup_steps, lr_min=self.lr_min)

    def is_default(self) -> bool:
        """a constant rate without warm-up: ``lr_at(t) == base_lr`` for every t"""
        return self.kind == "constant" and self.warmup_steps == 0


@dataclass(frozen=True)
class OptimConfig:
    """The options of a ``TrainEngine``'s update.  ``schedule``: None = the fixed ``hp.lr``; ``weight_decay``: AdamW's,
    0 = none; ``clip_grad``: ``clip_grad_norm_``'s ``max_norm`` per network, 0 = no clipping.  The default record is
    "everything off": an engine built with it is the engine built without one."""
    schedule: Optional[LRSchedule] = None
    weight_decay: float = 0.0
    clip_grad: float = 0.0

    def __post_init__(self):
        for name in ("weight_decay", "clip_grad"):
            v = float(getattr(self, name))
            if not (v >= 0.0 and math.isfinite(v)):
                raise ValueError(f"{name} {getattr(self, name)!r}: a finite value >= 0")

    def active(self) -> bool:
        """anything switched on (a constant schedule without warm-up at ``hp.lr`` counts: it is given, so it is used)"""
        return self.schedule is not None or self.weight_decay != 0.0 or self.clip_grad != 0.0

    def identity(self) -> Dict[str, Any]:
        """the keys a checkpoint's identity record gains: only what is not the default"""
        rec: Dict[str, Any] = {}
        if self.weight_decay != 0.0:
            rec["weight_decay"] = float(self.weight_decay)
        if self.clip_grad != 0.0:
            rec["clip_grad"] = float(self.clip_grad)
        if self.schedule is not None and not self.schedule.is_default():
            rec["lr_schedule"] = self.schedule.record()
        return rec


OPTIM_IDENTITY_KEYS = ("weight_decay", "clip_grad", "lr_schedule")
_OPTIM_DEFAULTS = {"weight_decay": 0.0, "clip_grad": 0.0, "lr_schedule": None}


def optim_identity_differences(saved: Dict[str, Any], mine: Dict[str, Any]):
    """the optimiser fields of two identity records that differ, by name (``lr_schedule.total_steps`` and its siblings
    one by one); an absent key is the default"""
    out = []
    for k in OPTIM_IDENTITY_KEYS:
        a, b = saved.get(k, _OPTIM_DEFAULTS[k]), mine.get(k, _OPTIM_DEFAULTS[k])
        if k != "lr_schedule":
            if a != b:
                out.append(f"{k}: file {a!r}, here {b!r}")
        elif a != b:
            if a is None or b is None:
                out.append(f"lr_schedule: file {'constant' if a is None else a['kind']!r}, "
                           f"here {'constant' if b is None else b['kind']!r}")
            else:
                for f in sorted(set(a) | set(b)):
                    if a.get(f) != b.get(f):
                        out.append(f"lr_schedule.{f}: file {a.get(f)!r}, here {b.get(f)!r}")
    return out


# ---------------------------------------------------------------------------- the definitions, in numpy
def live_ranges(param_off: Sequence[int], param_numel: Sequence[int]):
    """(offset, numel) of the ten live tensors of a flat block"""
    return [(int(param_off[t]), int(param_numel[t])) for t in range(NUM_LIVE)]


def grad_norm_host(grads, param_off, param_numel) -> Tuple[float, np.float32]:
    """(S, norm) of ONE network's flat gradient block: S = the fp64 sum of (double)g * (double)g over the ten live
    tensors, tensor by tensor -- the pad floats between tensors and the dead tensors do not count --, norm =
    float32(sqrt(S))"""
    g = np.asarray(grads).reshape(-1)
    S = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for off, n in live_ranges(param_off, param_numel):
            x = g[off:off + n].astype(np.float64)
            S += float(np.sum(x * x))
        return S, np.float32(np.sqrt(np.float64(S)))


def clip_coef_host(norm, max_norm) -> np.float32:
    """torch's ``clip_grad_norm_`` coefficient in fp32: ``max_norm / (norm + 1e-6)`` clamped to at most 1; a NaN norm
    gives NaN; ``max_norm == 0``: no clipping, 1"""
    max_norm = np.float32(max_norm)
    if max_norm == np.float32(0.0):
        return np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = np.float32(max_norm / np.float32(np.float32(norm) + np.float32(1e-6)))
    return np.float32(1.0) if c > np.float32(1.0) else c


def keep_host(lr, weight_decay) -> np.float32:
    """AdamW's decay factor: float32(1 - (double)lr * (double)weight_decay), of the fp32 ``lr`` and ``weight_decay``"""
    return np.float32(1.0 - float(np.float32(lr)) * float(np.float32(weight_decay)))


def adam_scalars_host(lr, beta1, beta2, t):
    """(step_size, bc2_sqrt) as cmlpl_dyn_adam forms them: in double from the fp32 hyper-parameters, rounded once"""
    lr, b1, b2 = float(np.float32(lr)), float(np.float32(beta1)), float(np.float32(beta2))
    return np.float32(lr / (1.0 - b1 ** t)), np.float32(math.sqrt(1.0 - b2 ** t))


def adamw_host(p, g, m, v, t: int, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, coef=1.0):
    """One clipped, decayed Adam step on fp32 arrays, every operation a rounded fp32 one in the order of the definition:
    g' = g * coef; p' = p * keep; then torch.optim.Adam's single-tensor update of (p', g').  Returns (p, m, v)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    step_size, bc2_sqrt = adam_scalars_host(lr, beta1, beta2, t)
    w1, w2 = f(1.0 - float(f(beta1))), f(1.0 - float(f(beta2)))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        g = g * f(coef)
        p = p * keep_host(lr, weight_decay)
        m = m + w1 * (g - m)                               # exp_avg.lerp_(grad, 1 - beta1)
        v = v * f(beta2) + (w2 * g) * g                    # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        denom = np.sqrt(v) / bc2_sqrt + f(eps)
        p = p - step_size * (m / denom)                    # param.addcdiv_(exp_avg, denom, -step_size)
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)
