#!/usr/bin/env python3
"""Drop-in for the reference's ``sample_generation.py`` (sample_generation.py:21-73, tools/hyper_tools.py:250-292): same
flags, same ``.mat`` files and keys, same ``./dataset/<name>/`` directory -- but the scene is z-scored and PCA'd on the
GPU (cmlpl_amd.scene, fp64 on the f64 MFMA) and NO ``XP.npy`` is written (19.9 GB for PaviaU at the defaults).  It writes
  X.npy (float64 z-scored spectra), Y.npy (the .mat label dtype), train_array.npy, test_array.npy, unlabel_array.npy
  in the reference's layout, plus
  cube.npy (float32 [rows, cols, n_PC], the z-scored PCA scene the windows are cut from) and scene.json (w, n_PC, rows,
  cols);
hsi_loader.HSIDataSet cuts the w x w windows from the cube (on the device for a whole split, one
cmlpl_extract_patches call).  The splits are the reference's, seeds and order included (cmlpl_amd.scene.make_splits)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# dataID: directory name, scene file, scene key, label file, label key (hyper_tools.py:250-276)
SCENES = {1: ("PaviaU", "PaviaU.mat", "paviaU", "PaviaU_gt.mat", "paviaU_gt"),
          2: ("Salinas", "salinas.mat", "HSI_original", "salinas_gt.mat", "Data_gt"),
          3: ("Houston", "Houston.mat", "Houston", "Houston_gt.mat", "Houston_gt"),
          4: ("Indian_pines", "indian_pines_corrected.mat", "indian_pines_corrected", "indian_pines_gt.mat",
              "indian_pines_gt")}


def load_mat(path, key):
    import scipy.io as sio
    try:
        return sio.loadmat(path)[key]
    except NotImplementedError:            # scipy's answer to a MATLAB v7.3 (HDF5) file
        raise SystemExit(f"error: {path} is a MATLAB v7.3 (HDF5) file, which scipy.io.loadmat cannot read; this script "
                         "has no HDF5 .mat reader (the reference uses hdf5storage). Save it again as a v7 .mat file "
                         "(MATLAB: save(name, var, '-v7')).")


def main(args):
    if args.dataID not in SCENES:
        raise SystemExit(f"error: --dataID {args.dataID}: known are {sorted(SCENES)}")
    w, n_PC = int(args.w), int(args.n_PC)
    if w < 2 or w % 2:
        raise SystemExit(f"error: --w {w}: the window must be even and at least 2 (the reference's ExtractPatches "
                         "cuts a (w-1) x (w-1) patch into a w x w slot for odd w)")
    if n_PC < 1:
        raise SystemExit(f"error: --n_PC {n_PC}: need at least one component")
    name, fx, kx, fy, ky = SCENES[args.dataID]
    X = load_mat(os.path.join("dataset", fx), kx)
    Y = load_mat(os.path.join("dataset", fy), ky)
    if X.ndim != 3 or Y.shape != X.shape[:2]:
        raise SystemExit(f"error: scene {X.shape} and labels {Y.shape} do not match")
    rows, cols, bands = X.shape
    if n_PC > bands:
        raise SystemExit(f"error: --n_PC {n_PC} > {bands} bands")
    if w // 2 > min(rows, cols):
        raise SystemExit(f"error: --w {w}: half the window exceeds the {rows} x {cols} scene (MirrowCut reflects once)")
    save_dir = os.path.join("dataset", name)
    if os.path.exists(os.path.join(save_dir, "XP.npy")):
        raise SystemExit(f"error: {save_dir}/XP.npy exists (written by the reference's preprocessing); hsi_loader reads "
                         "it in preference to the cube this script writes: delete it first")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("error: no GPU: the scene is built by the HIP kernels of cmlpl_amd (no CPU path)")
    from cmlpl_amd.scene import build_scene, make_splits

    cube, spectra = build_scene(X, n_PC, "cuda")
    train_array, test_array, unlabel_array = make_splits(Y, args.num_label)
    os.makedirs(save_dir, exist_ok=True)
    np.save(os.path.join(save_dir, "X.npy"), spectra.cpu().numpy())
    np.save(os.path.join(save_dir, "Y.npy"), Y.reshape(rows * cols))
    np.save(os.path.join(save_dir, "train_array.npy"), train_array)
    np.save(os.path.join(save_dir, "test_array.npy"), test_array)
    np.save(os.path.join(save_dir, "unlabel_array.npy"), unlabel_array)
    np.save(os.path.join(save_dir, "cube.npy"), cube.cpu().numpy())
    with open(os.path.join(save_dir, "scene.json"), "w") as f:
        json.dump({"w": w, "n_PC": n_PC, "rows": rows, "cols": cols}, f)
    print(f"{save_dir}: {rows} x {cols} x {bands} -> cube {rows} x {cols} x {n_PC}, window {w}; "
          f"train {len(train_array)}, test {len(test_array)}, unlabel {len(unlabel_array)}")


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--dataID', type=int, default=1)
    parser.add_argument('--num_label', type=int, default=5)
    parser.add_argument('--w', type=int, default=20)
    parser.add_argument('--n_PC', type=int, default=60)
    return parser


if __name__ == '__main__':
    main(build_parser().parse_args())
