"""Drop-in for the reference's ``hsi_loader.HSIDataSet`` (hsi_loader.py:5-133): same constructor and
item tuples -- (XP f32[C,w,w], X f32[bands], Y int) for 'label' / 'unlabel' / 'test', (XP, X) for
'wholeset' -- read from the ``.npy`` files ``sample_generation.py`` writes.  ``SyntheticHSIDataSet``
serves N(0,1) patches of any window shape when the datasets are not on disk (they are not shipped).
``device_arrays()`` hands the whole split to the GPU once: the training driver keeps it resident in
HBM and gathers batches by index there instead of copying 24.6 MB over PCIe per step.
A directory that this repository's ``sample_generation.py`` wrote has no XP.npy but ``cube.npy`` + ``scene.json``: the
windows are then cut from the cube (``CubeWindows``), with the same item tuples.  ``scene_arrays()`` hands such a split
to the GPU WITHOUT its windows -- spectra, labels and one scene pixel per row -- for the cube-fed training step, which
gathers the windows from the resident cube (``scene_cube``) itself."""
import json
import os

import numpy as np
import torch
from torch.utils import data

_ROOTS = {1: './dataset/PaviaU/', 2: './dataset/Salinas/', 3: './dataset/Houston/', 4: './dataset/Indian_pines/'}
_SCENES = {1: (610, 340), 2: (512, 217), 3: (349, 1905), 4: (145, 145)}       # rows, cols of the scenes train.py:75-90 names


def _tile_to(arr, max_iters):
    reps, rem = divmod(int(max_iters), len(arr))
    parts = [arr] * reps + ([arr[:rem]] if rem else [])
    return np.concatenate(parts) if parts else arr[:0]


def _mirror(i, n):
    """MirrowCut's reflection (tools/hyper_tools.py:35-55) of indices at most n outside [0, n)"""
    return np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))


def _scene_meta(root):
    path = root + 'scene.json'
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


class CubeWindows:
    """The w x w windows of the pixels ``idx`` (row-major pixel numbers) of a scene cube [rows, cols, C], cut on demand
    through the mirror index as tools/hyper_tools.py:226-243 ExtractPatches cuts them: stands where the rows of XP.npy
    stood.  ``shape`` is theirs, [n, C, w, w]; item i is the float32 window [C, w, w] of pixel idx[i]."""

    def __init__(self, cube, w, idx):
        self.cube, self.w, self.idx = cube, int(w), np.asarray(idx, dtype=np.int64)
        self.shape = (len(self.idx), cube.shape[2], self.w, self.w)

    def __len__(self):
        return len(self.idx)

    def cut(self, idx):
        """windows [len(idx), C, w, w] of the pixels idx, on the host"""
        rows, cols, _ = self.cube.shape
        r, c = np.divmod(np.asarray(idx, dtype=np.int64), cols)
        off = np.arange(self.w) - self.w // 2
        ri = _mirror(r[:, None] + off, rows)
        ci = _mirror(c[:, None] + off, cols)
        return np.moveaxis(np.asarray(self.cube[ri[:, :, None], ci[:, None, :]], dtype=np.float32), 3, 1)

    def __getitem__(self, index):
        return self.cut(self.idx[[index]])[0]

    def device_tensor(self, device):
        """all windows as one tensor on ``device``: ONE cmlpl_extract_patches call on a GPU"""
        device = torch.device(device)
        if device.type != 'cuda' or len(self.idx) == 0:
            return torch.from_numpy(self.cut(self.idx)).to(device)
        from cmlpl_amd.patches import extract_patches
        cube = torch.from_numpy(np.ascontiguousarray(self.cube, dtype=np.float32)).to(device)
        return extract_patches(cube, torch.from_numpy(self.idx).to(device), self.w)


class HSIDataSet(data.Dataset):
    def __init__(self, dataID, setindex='label', max_iters=None, num_unlabel=1000, root=None):
        self.setindex = setindex
        self.root = root or _ROOTS[int(dataID)]
        X = np.load(self.root + 'X.npy', mmap_mode='r')
        Y = np.load(self.root + 'Y.npy') - 1
        if os.path.exists(self.root + 'XP.npy'):
            XP = np.load(self.root + 'XP.npy', mmap_mode='r')
        else:
            meta = _scene_meta(self.root)
            if meta is None:
                raise FileNotFoundError(f"{self.root}: neither XP.npy nor cube.npy + scene.json (sample_generation.py)")
            XP = CubeWindows(np.load(self.root + 'cube.npy', mmap_mode='r'), meta['w'], np.arange(len(X)))
        if setindex == 'wholeset':
            self.XP, self.X, self.Y = XP, X, None
            return
        fname = {'label': 'train_array.npy', 'unlabel': 'unlabel_array.npy', 'test': 'test_array.npy'}[setindex]
        idx = np.load(self.root + fname)
        if setindex == 'unlabel':
            idx = idx[:num_unlabel]
        if isinstance(XP, CubeWindows):
            if max_iters is not None and setindex in ('label', 'unlabel'):
                idx = _tile_to(idx, max_iters)
            self.XP, self.X, self.Y = CubeWindows(XP.cube, XP.w, idx), np.asarray(X[idx]), Y[idx]
            return
        self.XP, self.X, self.Y = np.asarray(XP[idx]), np.asarray(X[idx]), Y[idx]
        if max_iters is not None and setindex in ('label', 'unlabel'):
            self.XP, self.X, self.Y = (_tile_to(a, max_iters) for a in (self.XP, self.X, self.Y))

    def __len__(self):
        return len(self.X)

    def __getitem__(self, index):
        XP = np.array(self.XP[index], dtype=np.float32)
        X = np.array(self.X[index], dtype=np.float32)
        if self.Y is None:
            return XP, X
        return XP, X, int(self.Y[index])

    def device_arrays(self, device):
        if isinstance(self.XP, CubeWindows):
            XP = self.XP.device_tensor(device)
        else:
            XP = torch.from_numpy(np.ascontiguousarray(self.XP, dtype=np.float32)).to(device)
        X = torch.from_numpy(np.ascontiguousarray(self.X, dtype=np.float32)).to(device)
        Y = None if self.Y is None else torch.from_numpy(np.asarray(self.Y, dtype=np.int64)).to(device)
        return XP, X, Y

    @property
    def scene_cube(self):
        """the scene [rows, cols, C] the split's windows are cut from (cube.npy, memory-mapped); None for a directory
        with a materialised XP.npy"""
        return self.XP.cube if isinstance(self.XP, CubeWindows) else None

    def scene_arrays(self, device):
        """(X, Y, pix) on ``device`` for the cube-fed step: row i of the split is the window ``CubeWindows.cut(pix[i])``
        of ``scene_cube`` with spectrum X[i] and label Y[i] -- the items of ``__getitem__``, tiled / truncated alike --
        and no window is cut.  Needs a split that came from cube.npy."""
        if not isinstance(self.XP, CubeWindows):
            raise ValueError(f"{self.root}: the split was read from XP.npy; scene_arrays() needs cube.npy + scene.json "
                             "(this repository's sample_generation.py)")
        X = torch.from_numpy(np.ascontiguousarray(self.X, dtype=np.float32)).to(device)
        Y = None if self.Y is None else torch.from_numpy(np.asarray(self.Y, dtype=np.int64)).to(device)
        return X, Y, torch.from_numpy(np.ascontiguousarray(self.XP.idx)).to(device)

    def cube_source(self, device, scene=None, dataID=None, resident_cube=None):
        """The 'wholeset' as the scene it was cut from, for whole-image inference without the materialised patches
        (tools.hyper_tools.test_whole): ``cube.npy`` ([rows, cols, C], the z-scored / PCA'd scene the patches were cut
        from: this repository's sample_generation.py writes it, with scene.json) next to XP.npy or in its place.  None
        when it is not there (the caller then streams the materialised patches, as the reference does): the cube is
        NOT rebuilt from XP.npy -- that gather touches every page of a ~20 GB file to recover 0.25 % of it.  The scene
        shape comes from scene.json when there is one (then any scene is taken), else from ``_SCENES``.
        ``resident_cube``: the same cube.npy already on ``device`` (a cube-fed training run keeps it there): used in
        place of a second upload."""
        from cmlpl_amd.infer import CubeSource
        if self.setindex != 'wholeset':
            raise ValueError("cube_source() is for the 'wholeset'")
        path = self.root + 'cube.npy'
        if not os.path.exists(path):
            return None
        cube = np.load(path, mmap_mode='r')
        meta = _scene_meta(self.root)
        if scene is None and meta is not None:
            scene = (int(meta['rows']), int(meta['cols']))
        elif scene is None and dataID is not None:
            scene = _SCENES.get(int(dataID))
        if cube.ndim != 3 or (scene is not None and tuple(cube.shape[:2]) != tuple(scene)):
            return None
        if resident_cube is not None and tuple(resident_cube.shape) == tuple(cube.shape):
            cube = resident_cube
        else:
            cube = torch.from_numpy(np.ascontiguousarray(cube, dtype=np.float32)).to(device)
        X = torch.from_numpy(np.ascontiguousarray(self.X, dtype=np.float32)).to(device)
        if cube.shape[0] * cube.shape[1] != X.shape[0]:
            return None
        return CubeSource(cube, X)


class SyntheticHSIDataSet(data.Dataset):
    """Seeded stand-in with the same item tuples; class-dependent mean so that training has signal.
    ``scene`` (a ``SyntheticScene``): the split is then ``length`` seeded pixels of that scene -- windows cut from its
    cube as ``HSIDataSet`` cuts them from cube.npy, spectra and labels the pixels' own -- and ``scene_arrays()`` serves
    the cube-fed step."""

    def __init__(self, shape, length, setindex='label', seed=1088, separable=1.0, scene=None):
        C, H, W, bands, K = shape
        g = torch.Generator().manual_seed(seed)
        self.setindex, self.scene = setindex, scene
        if scene is not None:
            if H != W or scene.cube.shape[2] != C or scene.X.shape[1] != bands:
                raise ValueError("the scene does not carry this shape's windows")
            self.pix = torch.randint(0, len(scene), (length,), generator=g)
            self.Y, self.X = scene.Y[self.pix], scene.X[self.pix]
            self.XP = CubeWindows(scene.cube.numpy(), H, self.pix.numpy())
            return
        proto_g = torch.Generator().manual_seed(4242)
        self.Y = torch.randint(0, K, (length,), generator=g)
        proto_p = torch.randn(K, C, 1, 1, generator=proto_g) * separable
        proto_x = torch.randn(K, bands, generator=proto_g) * separable
        self.XP = torch.randn(length, C, H, W, generator=g) + proto_p[self.Y]
        self.X = torch.randn(length, bands, generator=g) + proto_x[self.Y]

    def __len__(self):
        return len(self.X)

    def __getitem__(self, index):
        XP = self.XP[index] if self.scene is not None else self.XP[index].numpy()
        if self.setindex == 'wholeset':
            return XP, self.X[index].numpy()
        return XP, self.X[index].numpy(), int(self.Y[index])

    def device_arrays(self, device):
        if self.scene is not None:
            return self.XP.device_tensor(device), self.X.to(device), self.Y.to(device)
        return self.XP.to(device), self.X.to(device), self.Y.to(device)

    @property
    def scene_cube(self):
        return None if self.scene is None else self.scene.cube

    def scene_arrays(self, device):
        """(X, Y, pix) on ``device``, as ``HSIDataSet.scene_arrays``; needs the ``scene`` the split was drawn from"""
        if self.scene is None:
            raise ValueError("scene_arrays() needs a split drawn from a SyntheticScene (scene=)")
        return self.X.to(device), self.Y.to(device), self.pix.to(device)


class SyntheticScene:
    """A seeded synthetic scene for whole-image inference: a cube [rows, cols, C] and spectra [rows * cols, bands] whose
    pixels carry the class-dependent means of ``SyntheticHSIDataSet`` (same prototypes), plus the per-pixel labels.
    The classes lie in square REGIONS one and a half windows wide (a real scene's fields and roofs; each region its own
    seeded class), so that a window is mostly one class, like the training patches, which carry one class mean over the
    whole window -- with a class per pixel the spatial branch met windows it never trained on."""

    def __init__(self, shape, rows, cols, seed=3, separable=1.0):
        C, H, W, bands, K = shape
        g = torch.Generator().manual_seed(seed)
        proto_g = torch.Generator().manual_seed(4242)
        self.rows, self.cols, self.window = int(rows), int(cols), H
        blk = max(1, (3 * H) // 2)
        nbr, nbc = (rows + blk - 1) // blk, (cols + blk - 1) // blk
        region = torch.randint(0, K, (nbr, nbc), generator=g)
        self.Y = region.repeat_interleave(blk, 0)[:rows].repeat_interleave(blk, 1)[:, :cols].reshape(-1).contiguous()
        proto_p = torch.randn(K, C, 1, 1, generator=proto_g) * separable
        proto_x = torch.randn(K, bands, generator=proto_g) * separable
        self.cube = (torch.randn(rows * cols, C, generator=g) + proto_p[self.Y].view(-1, C)).view(rows, cols, C)
        self.X = torch.randn(rows * cols, bands, generator=g) + proto_x[self.Y]

    def __len__(self):
        return self.rows * self.cols

    def cube_source(self, device, resident_cube=None):
        """``resident_cube``: this scene's cube already on ``device`` (a cube-fed training run keeps it there)"""
        from cmlpl_amd.infer import CubeSource
        cube = resident_cube if resident_cube is not None else self.cube.to(device).contiguous()
        return CubeSource(cube, self.X.to(device).contiguous())
