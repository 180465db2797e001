#!/usr/bin/env python3
"""Fixture for the preprocessing row (sample_generation.py): write two tiny seeded scenes as .mat files in
a temporary cwd, run the REFERENCE sample_generation.main on them (reference sample_generation.py:21-73 with
tools/hyper_tools.py, loaded by file path), and store what it writes plus the unrounded cube of its PCANorm /
featureNormalize.  (Named patches_*: tests/golden_util.golden_cases() takes every other npz for a step trajectory.)
Build container only:
    python tests/golden/make_golden_samplegen.py
Per case <c> the npz holds: <c>_raw (the scene as saved), <c>_gt, <c>_cfg (dataID, w, n_PC, num_label), <c>_X, <c>_Y,
<c>_train / _test / _unlabel, <c>_cube (fp64 [rows, cols, n_PC]), <c>_xp_idx + <c>_xp (XP rows at corner / edge / random
pixels), <c>_xp_sum (fp64 per-channel sums of the whole XP) and <c>_xp_sha (sha256 of the whole XP as C-ordered float32).
  a: PaviaU keys, uint16, 31 x 23 x 24, w 12, n_PC 6, every pixel labelled;
  b: Houston keys, float32, 64 x 64 x 16, w 8, n_PC 6, 300 labelled pixels: the unlabel order (CPython set order)
     is not sorted there.  The float32 values are multiples of 1/64 in [640, 2400] with a band mean in [1024, 2048):
     the reference's float32 `X - mean(X)` (PCANorm, hyper_tools.py:26-27) is then exact, so its cube is the fp64 math.
     Its X.npy is float32 (featureNormalize in float32): <c>_X is that file as written."""
import hashlib
import os
import sys
import tempfile

import numpy as np
import scipy.io as sio

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden._refload import load_reference_module  # noqa: E402

KEYS = {1: ("PaviaU", "PaviaU.mat", "paviaU", "PaviaU_gt.mat", "paviaU_gt"),
        3: ("Houston", "Houston.mat", "Houston", "Houston_gt.mat", "Houston_gt")}


def low_rank(rng, rows, cols, bands, scales, noise):
    """a scene whose covariance has well separated leading eigenvalues: sum_k s_k a_k v_k^T + noise"""
    V = np.linalg.qr(rng.standard_normal((bands, bands)))[0][:, :len(scales)]
    A = rng.standard_normal((rows * cols, len(scales))) * np.asarray(scales)
    return (A @ V.T + noise * rng.standard_normal((rows * cols, bands))).reshape(rows, cols, bands)


def case_a():
    rng = np.random.Generator(np.random.PCG64(11))
    rows, cols, bands = 31, 23, 24
    x = 3000 + low_rank(rng, rows, cols, bands, [600, 380, 240, 150, 95, 60, 38], 4.0)
    raw = np.clip(np.rint(x), 0, 65535).astype(np.uint16)
    gt = rng.integers(1, 6, size=(rows, cols)).astype(np.uint8)
    return raw, gt, dict(dataID=1, w=12, n_PC=6, num_label=5)


def case_b():
    rng = np.random.Generator(np.random.PCG64(12))
    rows, cols, bands = 64, 64, 16
    x = 1500 + low_rank(rng, rows, cols, bands, [160, 110, 75, 50, 33, 22, 15], 2.0)
    raw = (np.rint(np.clip(x, 640, 2400) * 64) / 64).astype(np.float32)
    gt = np.zeros(rows * cols, dtype=np.uint8)
    lab = rng.choice(rows * cols, size=300, replace=False)
    gt[lab] = rng.integers(1, 8, size=300)
    return raw, gt.reshape(rows, cols), dict(dataID=3, w=8, n_PC=6, num_label=10)


def xp_pixels(rows, cols, rng):
    corners = [0, cols - 1, (rows - 1) * cols, rows * cols - 1]
    edges = [cols // 2, (rows // 2) * cols, (rows // 2) * cols + cols - 1, (rows - 1) * cols + cols // 3]
    return np.array(corners + edges + sorted(rng.choice(rows * cols, size=8, replace=False).tolist()), dtype=np.int64)


def run_reference(sg, hyper, raw, gt, cfg):
    name, fx, kx, fy, ky = KEYS[cfg["dataID"]]
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        os.chdir(tmp)                       # the reference opens './dataset/...' relative to the cwd
        try:
            os.makedirs("dataset")
            sio.savemat(os.path.join("dataset", fx), {kx: raw})
            sio.savemat(os.path.join("dataset", fy), {ky: gt})

            class Args:
                dataID, w, n_PC, num_label = cfg["dataID"], cfg["w"], cfg["n_PC"], cfg["num_label"]
            sg.main(Args)
            d = os.path.join("dataset", name)
            out = {k: np.load(os.path.join(d, k + ".npy")) for k in ("XP", "X", "Y")}
            for k in ("train", "test", "unlabel"):
                out[k] = np.load(os.path.join(d, k + "_array.npy"))
        finally:
            os.chdir(cwd)
    rows, cols, bands = raw.shape
    X = raw.reshape(rows * cols, bands)
    out["cube"] = hyper.featureNormalize(hyper.PCANorm(X, cfg["n_PC"]), 1).reshape(rows, cols, cfg["n_PC"])
    return out


def main():
    saved = sys.modules.get("tools.hyper_tools")
    hyper = load_reference_module("tools/hyper_tools.py", "ref_hyper_tools")
    sys.modules["tools.hyper_tools"] = hyper          # sample_generation.py does `from tools.hyper_tools import *`
    try:
        sg = load_reference_module("sample_generation.py", "ref_sample_generation")
    finally:
        if saved is None:
            sys.modules.pop("tools.hyper_tools", None)
        else:
            sys.modules["tools.hyper_tools"] = saved
    out = {}
    for c, make in (("a", case_a), ("b", case_b)):
        raw, gt, cfg = make()
        r = run_reference(sg, hyper, raw, gt, cfg)
        rows, cols = raw.shape[:2]
        idx = xp_pixels(rows, cols, np.random.Generator(np.random.PCG64(5)))
        out.update({f"{c}_raw": raw, f"{c}_gt": gt, f"{c}_X": r["X"], f"{c}_Y": r["Y"], f"{c}_cube": r["cube"],
                    f"{c}_train": r["train"], f"{c}_test": r["test"], f"{c}_unlabel": r["unlabel"],
                    f"{c}_cfg": np.array([cfg["dataID"], cfg["w"], cfg["n_PC"], cfg["num_label"]], dtype=np.int64),
                    f"{c}_xp_idx": idx, f"{c}_xp": r["XP"][idx],
                    f"{c}_xp_sum": r["XP"].astype(np.float64).sum(axis=(0, 2, 3)),
                    f"{c}_xp_sha": np.array(hashlib.sha256(np.ascontiguousarray(r["XP"], np.float32).tobytes()).hexdigest())})
        u = r["unlabel"]
        print(c, raw.shape, raw.dtype, "XP", r["XP"].shape, "X", r["X"].dtype, "train/test/unlabel",
              len(r["train"]), len(r["test"]), len(u), "unlabel descents", int(np.sum(np.diff(u) < 0)))
    path = os.path.join(HERE, "patches_samplegen_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KB)")


if __name__ == "__main__":
    main()
