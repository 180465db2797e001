"""Shared by the preprocessing tests (CPU and GPU): the two cases of tests/golden/patches_samplegen_ref.npz (written by
tests/golden/make_golden_samplegen.py from the REFERENCE sample_generation.py) and the .mat files they came from."""
import os

import numpy as np
import scipy.io as sio

from tests.golden_util import GOLDEN_DIR

CASES = ("a", "b")
KEYS = {1: ("PaviaU", "PaviaU.mat", "paviaU", "PaviaU_gt.mat", "paviaU_gt"),
        3: ("Houston", "Houston.mat", "Houston", "Houston_gt.mat", "Houston_gt")}


def load_case(c):
    z = np.load(os.path.join(GOLDEN_DIR, "patches_samplegen_ref.npz"))
    d = {k[2:]: z[k] for k in z.files if k.startswith(c + "_")}
    d["dataID"], d["w"], d["n_PC"], d["num_label"] = (int(v) for v in d["cfg"])
    return d


def write_mats(cwd, dataID, raw, gt):
    """./dataset/<scene>.mat + <labels>.mat under cwd, with the reference's file names and keys"""
    _, fx, kx, fy, ky = KEYS[dataID]
    os.makedirs(os.path.join(cwd, "dataset"), exist_ok=True)
    sio.savemat(os.path.join(cwd, "dataset", fx), {kx: raw})
    sio.savemat(os.path.join(cwd, "dataset", fy), {ky: gt})
    return os.path.join(cwd, "dataset", KEYS[dataID][0])


def ulp_report(name, got, ref32, abs_floor=0.0):
    """|got - ref| <= max(spacing(|ref|), abs_floor) elementwise for float32 arrays; returns the fraction that differ"""
    got = np.asarray(got, dtype=np.float32)
    ref32 = np.asarray(ref32, dtype=np.float32)
    assert got.shape == ref32.shape, (name, got.shape, ref32.shape)
    d = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
    bound = np.maximum(np.spacing(np.abs(ref32)).astype(np.float64), abs_floor)
    bad = ~(d <= bound)
    frac = float(np.mean(got != ref32))
    print(f"{name}: {frac:.2e} of {got.size} differ (at most 1 ulp: {not bad.any()}), max |diff| {d.max():.3e}")
    assert not bad.any(), f"{name}: {int(bad.sum())} elements beyond 1 fp32 ulp, first at {np.argwhere(bad)[0]}"
    return frac
