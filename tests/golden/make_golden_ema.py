#!/usr/bin/env python3
"""Golden vectors for tools.models.WeightEMA_BN (the EMA teacher's update): run the reference's own function
(tools/models.py:155-164, CPU fp32 tensors) on a pair of tiny modules -- two Linear layers (7 -> 5, 5 -> 3), one
4,099-element parameter whose magnitudes span 1e-6 .. 1e3 and an int64 buffer -- four successive calls with Base
perturbed in between, at alpha 0.95 and 0.999; store Base before every call and Ensemble before the first and after
every call.  Build container only:  python tests/golden/make_golden_ema.py"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden._refload import load_reference_module  # noqa: E402

ref = load_reference_module("tools/models.py", "ref_models")
CALLS = 4


class Tiny(nn.Module):
    def __init__(self, rng):
        super().__init__()
        self.l1, self.l2 = nn.Linear(7, 5), nn.Linear(5, 3)
        self.wide = nn.Parameter(torch.zeros(4099))
        self.register_buffer("count", torch.tensor(0, dtype=torch.int64))
        with torch.no_grad():
            for p in (self.l1.weight, self.l1.bias, self.l2.weight, self.l2.bias):
                p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)))
            mag = 10.0 ** rng.uniform(-6.0, 3.0, 4099)
            self.wide.copy_(torch.from_numpy((rng.choice([-1.0, 1.0], 4099) * mag).astype(np.float32)))
            self.count.fill_(int(rng.integers(3, 1000)))


def snap(m):
    return {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}


os.makedirs(os.path.join(HERE, "ema"), exist_ok=True)
for tag, alpha, seed in (("a95", 0.95, 71), ("a999", 0.999, 72)):
    rng = np.random.Generator(np.random.PCG64(seed))
    base, ens = Tiny(rng), Tiny(rng)
    out = {"alpha": np.array([alpha], dtype=np.float64), "calls": np.array([CALLS], dtype=np.int64)}
    out.update({f"ens0.{k}": v for k, v in snap(ens).items()})
    for c in range(1, CALLS + 1):
        with torch.no_grad():                       # Base moves between the calls, as an optimiser would move it
            for p in base.parameters():
                p.mul_(torch.from_numpy((1.0 + 0.05 * rng.standard_normal(tuple(p.shape))).astype(np.float32)))
                p.add_(torch.from_numpy((1e-3 * rng.standard_normal(tuple(p.shape))).astype(np.float32)))
            base.count.add_(int(rng.integers(1, 50)))
        out.update({f"base{c}.{k}": v for k, v in snap(base).items()})
        got = ref.WeightEMA_BN(base, ens, alpha)
        assert got is ens
        out.update({f"ens{c}.{k}": v for k, v in snap(ens).items()})
    np.savez_compressed(os.path.join(HERE, "ema", tag + ".npz"), **out)
    print(tag, len(out), "arrays")
