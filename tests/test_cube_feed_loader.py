"""CPU: `scene_arrays()` of the loaders -- a split handed over WITHOUT its windows (spectra, labels, one scene pixel per
row) for the cube-fed training step -- against the items `__getitem__` serves from the same directory (written the way
tests/samplegen_util.py's fixture directories are written: cube.npy + scene.json, no XP.npy)."""
import json
import os

import numpy as np
import pytest

from tests.samplegen_util import CASES, KEYS, load_case


def _cube_dir(tmp_path, d):
    root = os.path.join(str(tmp_path), "dataset", KEYS[d["dataID"]][0]) + "/"
    os.makedirs(root)
    rows, cols, n_pc = d["cube"].shape
    np.save(root + "cube.npy", d["cube"].astype(np.float32))
    np.save(root + "X.npy", d["X"])
    np.save(root + "Y.npy", d["Y"])
    for k in ("train", "test", "unlabel"):
        np.save(root + k + "_array.npy", d[k])
    with open(root + "scene.json", "w") as f:
        json.dump({"w": d["w"], "n_PC": n_pc, "rows": rows, "cols": cols}, f)
    return root


@pytest.mark.parametrize("c", CASES)
def test_scene_arrays_name_the_items_of_the_split(tmp_path, c):
    from hsi_loader import HSIDataSet
    d = load_case(c)
    root = _cube_dir(tmp_path, d)
    rows, cols, n_pc = d["cube"].shape
    for setindex, max_iters, num_unlabel in (("label", 2 * len(d["train"]) + 3, 1000),      # tiled to max_iters
                                             ("unlabel", None, 37),                         # truncated by num_unlabel
                                             ("unlabel", 100, 37)):                         # truncated, then tiled
        ds = HSIDataSet(d["dataID"], setindex, max_iters=max_iters, num_unlabel=num_unlabel, root=root)
        X, Y, pix = ds.scene_arrays("cpu")
        assert tuple(ds.scene_cube.shape) == (rows, cols, n_pc)
        assert pix.dtype.is_floating_point is False and pix.numpy().dtype == np.int64
        assert len(pix) == len(X) == len(Y) == len(ds)
        assert int(pix.min()) >= 0 and int(pix.max()) < rows * cols
        for i in range(len(ds)):
            xp, x, y = ds[i]
            assert np.array_equal(ds.XP.cut(pix[i:i + 1].numpy())[0], xp)
            assert np.array_equal(X[i].numpy(), x) and int(Y[i]) == y


def test_scene_arrays_need_the_cube(tmp_path, monkeypatch):
    """a directory with a materialised XP.npy has no scene to gather from: the method says so"""
    from hsi_loader import HSIDataSet
    from tests.hsiloader_util import make_tiny_dataset
    monkeypatch.chdir(tmp_path)
    make_tiny_dataset("./dataset/PaviaU/")
    ds = HSIDataSet(1, "label", max_iters=11)
    assert ds.scene_cube is None
    with pytest.raises(ValueError, match="cube.npy"):
        ds.scene_arrays("cpu")


def test_synthetic_split_of_a_scene():
    from hsi_loader import SyntheticHSIDataSet, SyntheticScene
    shape = (6, 4, 4, 5, 3)
    scene = SyntheticScene(shape, 9, 7, seed=3)
    ds = SyntheticHSIDataSet(shape, 20, "label", seed=1, scene=scene)
    X, Y, pix = ds.scene_arrays("cpu")
    XP, X2, Y2 = ds.device_arrays("cpu")
    assert tuple(XP.shape) == (20, 6, 4, 4) and np.array_equal(X.numpy(), X2.numpy()) and np.array_equal(Y.numpy(), Y2.numpy())
    for i in range(20):
        xp, x, y = ds[i]
        assert np.array_equal(ds.XP.cut(pix[i:i + 1].numpy())[0], xp) and np.array_equal(XP[i].numpy(), xp)
        assert np.array_equal(x, scene.X[pix[i]].numpy()) and y == int(scene.Y[pix[i]])
    with pytest.raises(ValueError):
        SyntheticHSIDataSet(shape, 20, "label", seed=1).scene_arrays("cpu")
