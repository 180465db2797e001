"""The training dataset from the raw scene (reference sample_generation.py:21-73, tools/hyper_tools.py:8-32,285-292
``SampleGen``) without ``XP.npy``: the z-scored PCA cube and the z-scored spectra are computed on the device
(``cmlpl_scene_gram`` / ``cmlpl_scene_project``, fp64 on the f64 MFMA), the windows are cut from the cube when they are
needed (``cmlpl_extract_patches``).  Only the bands x bands SVD runs on the host, through the same LAPACK call the
reference makes, so that the components keep the reference's signs.  ``make_splits`` is the reference's split logic."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

# .mat dtypes the kernels read as they are (converted exactly to fp64 in the kernel); other numeric dtypes are
# converted to fp64 on the host first
_DTYPES = {np.dtype(np.uint16): 0, np.dtype(np.int16): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}
MAX_BANDS = 256


def _check(raw: np.ndarray, n_PC: int):
    if not isinstance(raw, np.ndarray) or raw.ndim != 3:
        raise ValueError("raw: need a numpy array [rows, cols, bands]")
    if raw.dtype == np.bool_ or not np.issubdtype(raw.dtype, np.number) or np.issubdtype(raw.dtype, np.complexfloating):
        raise ValueError(f"raw: dtype {raw.dtype} is not a real numeric type")
    rows, cols, bands = raw.shape
    if rows * cols < 2:
        raise ValueError(f"raw: a scene needs at least 2 pixels, got {rows} x {cols}")
    if not 1 <= bands <= MAX_BANDS:
        raise ValueError(f"raw: {bands} bands, the kernels take 1 .. {MAX_BANDS}")
    if not 1 <= int(n_PC) <= bands:
        raise ValueError(f"n_PC = {n_PC}: need 1 <= n_PC <= bands = {bands}")


def _upload(raw: np.ndarray, device):
    """the scene on the device as [pixels, bands] in a dtype the kernels read, and that dtype's code"""
    if raw.dtype not in _DTYPES:
        raw = raw.astype(np.float64)
    flat = np.ascontiguousarray(raw).reshape(-1, raw.shape[-1])
    code = _DTYPES[raw.dtype]
    host = flat.view(np.int16) if code == 0 else flat      # uint16 travels as its bits
    return torch.from_numpy(host).to(device), code


def _workspace(pixels, bands, n_pc, device):
    nbytes = _lib.load().cmlpl_scene_workspace_bytes(int(pixels), int(bands), int(n_pc))
    if nbytes == 0:
        raise ValueError(f"scene of {pixels} pixels x {bands} bands, n_PC = {n_pc}: not a shape the kernels take")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def scene_gram(d_raw: torch.Tensor, code: int, ws: torch.Tensor):
    """(mean [bands], G [bands, bands]) fp64 cuda of the scene d_raw [pixels, bands] (as ``_upload`` leaves it):
    G = (X - mean)^T (X - mean); np.cov of the reference's PCANorm is G / (pixels - 1).  Asynchronous."""
    n, bands = d_raw.shape
    mean = torch.empty(bands, dtype=torch.float64, device=d_raw.device)
    gram = torch.empty(bands, bands, dtype=torch.float64, device=d_raw.device)
    _lib.check("cmlpl_scene_gram", _lib.load().cmlpl_scene_gram(
        d_raw.data_ptr(), code, n, bands, mean.data_ptr(), gram.data_ptr(), ws.data_ptr(), ws.numel(),
        _lib.stream(d_raw.device)))
    return mean, gram


def pca_basis(gram: np.ndarray, pixels: int, n_PC: int) -> np.ndarray:
    """U[:, :n_PC] of the reference's ``np.linalg.svd(np.cov(X_norm.T))`` (hyper_tools.py:29-30), from G"""
    U = np.linalg.svd(np.asarray(gram, dtype=np.float64) / (pixels - 1))[0]
    return np.ascontiguousarray(U[:, :n_PC])


def scene_project(d_raw: torch.Tensor, code: int, mean: torch.Tensor, gram: torch.Tensor, basis: torch.Tensor,
                  ws: torch.Tensor, spectra: bool = True):
    """(cube f32 [pixels, n_PC], spectra f64 [pixels, bands] or None) from the scene and its basis.  Asynchronous."""
    n, bands = d_raw.shape
    n_pc = basis.shape[1]
    cube = torch.empty(n, n_pc, dtype=torch.float32, device=d_raw.device)
    spec = torch.empty(n, bands, dtype=torch.float64, device=d_raw.device) if spectra else None
    _lib.check("cmlpl_scene_project", _lib.load().cmlpl_scene_project(
        d_raw.data_ptr(), code, n, bands, mean.data_ptr(), gram.data_ptr(), basis.data_ptr(), n_pc, cube.data_ptr(),
        _lib.ptr(spec), ws.data_ptr(), ws.numel(), _lib.stream(d_raw.device)))
    return cube, spec


def build_scene(raw: np.ndarray, n_PC: int, device="cuda"):
    """(cube float32 cuda [rows, cols, n_PC], spectra float64 cuda [rows * cols, bands]) of the raw scene
    raw [rows, cols, bands]: ``featureNormalize(PCANorm(X, n_PC), 1)`` rounded once to fp32, and ``featureNormalize(X, 1)``
    (hyper_tools.py:285-292).  Raises ValueError before any launch for a scene the kernels do not take."""
    _check(raw, n_PC)
    rows, cols, bands = raw.shape
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"build_scene runs on a GPU, not on {device}")
    d_raw, code = _upload(raw, device)
    ws = _workspace(rows * cols, bands, n_PC, device)
    mean, gram = scene_gram(d_raw, code, ws)
    basis = torch.from_numpy(pca_basis(gram.cpu().numpy(), rows * cols, n_PC)).to(device)
    cube, spectra = scene_project(d_raw, code, mean, gram, basis, ws)
    return cube.view(rows, cols, n_PC), spectra


def make_splits(Y, num_label: int):
    """(train, test, unlabel) pixel indices of sample_generation.py:45-65 for the labels Y (0 = unlabelled, classes
    1 .. max): the labelled pixels shuffled with seed 2; per class a seed-0 permutation whose first ``num_label`` pixels
    train and the rest test; ``unlabel`` = the shuffled labelled pixels minus the training ones, in the order of
    ``list(set(.) - set(.))`` -- CPython's hash-table order, which decides which pixels ``--num_unlabel`` keeps, so it is
    produced by that same set operation.  numpy's global random state is left alone."""
    Y = np.asarray(Y).reshape(-1)
    whole = np.where(Y > 0)[0]
    np.random.RandomState(2).shuffle(whole)
    train, test = [], []
    for i in range(1, int(Y.max()) + 1):
        index = np.where(Y == i)[0]
        perm = np.random.RandomState(0).permutation(index.shape[0])
        train.append(index[perm[0:num_label]])
        test.append(index[perm[num_label:]])
    train = np.concatenate(train) if train else np.zeros(0, dtype=np.int64)
    test = np.concatenate(test) if test else np.zeros(0, dtype=np.int64)
    unlabel = np.array(list(set(whole) - set(train)))
    return train, test, unlabel
