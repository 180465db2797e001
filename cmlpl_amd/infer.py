"""Whole-image inference straight from the scene cube (reference tools/hyper_tools.py:416-437 ``test_whole`` over the
patches of :226-243 ``ExtractPatches``; train.py:291-294).  The reference materialises every pixel's window (19.9 GB
for PaviaU) and streams it through a DataLoader; here the z-scored / PCA'd cube [rows, cols, C] and the spectra
[rows * cols, bands] stay resident in HBM and ``cmlpl_infer_cube`` gathers each window through the mirror index while
the fused forward stages its input slab -- no patch tensor exists, the argmax is written on the device."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib


class CubeSource(NamedTuple):
    """what ``tools.hyper_tools.test_whole`` takes instead of a DataLoader of patches"""
    cube: torch.Tensor          # [rows, cols, C] float32 cuda, band-last (the scene the patches are cut from)
    spectra: torch.Tensor       # [rows * cols, bands] float32 cuda (row-major pixel order)


def _net_buffers(net):
    """(shape struct, flat parameters, packed weights) of ONE network: a cmlpl_amd.models.BaseNet2 module, or a
    (TrainEngine, net index) pair."""
    if isinstance(net, tuple):
        eng, i = net
        eng._ensure_packed(_lib.stream(eng.device))
        return eng.cshape, eng.params[i], eng.packed[i]
    flat, packed = net._flat_params(net._live_params())
    return net._cshape, flat, packed


def infer_fused(shape) -> bool:
    """does ``cmlpl_infer_cube`` -- the fused eval forward that gathers the window while it stages its slab -- take this
    window shape?  (square windows of 8 x 8 up to 256 pixels whose final pooled map the per-sample fused forward covers;
    asked of the library: its workspace size is 0 otherwise)"""
    lib = _lib.load()
    cs = _lib.Shape(shape.C, shape.H, shape.W, shape.bands, shape.K)
    return lib.cmlpl_infer_workspace_bytes(C.byref(cs), 8) > 0


def infer_supported(shape) -> bool:
    """can ``infer_cube`` label a scene of this window shape straight from its cube?  Every square window the network
    runs on: the fused kernel where it applies (``infer_fused``), else -- the reference's own 20 x 20 x 60 windows -- the
    windows of a few thousand pixels at a time cut on the device (cmlpl_extract_patches) and run through the general
    forward (cmlpl_basenet2_fwd).  Either way the scene stays in HBM as its cube; the 19.9 GB patch tensor never exists.
    By patches one window has to fit the cut's LDS (``cmlpl_patches_fit``: about w * w * C <= 40,960 -- 101 channels at
    20 x 20), for the clean cut and the view cut alike: ``infer_cube``, the ensemble and TTA answer to the same promise."""
    lib = _lib.load()
    cs = _lib.Shape(shape.C, shape.H, shape.W, shape.bands, shape.K)
    if shape.H != shape.W or lib.cmlpl_workspace_bytes(C.byref(cs), 1, 8, 8) == 0:
        return False
    return infer_fused(shape) or lib.cmlpl_patches_fit(shape.C, shape.H) == 3


def _nets_buffers(nets):
    """(shape struct, n networks, parameters, parameter stride, packed weights, packed stride, squeeze) of what
    ``infer_pixels`` was given: ONE network as ``_net_buffers`` takes it (a BaseNet2 module or (TrainEngine, index)) --
    then the results carry no network dimension --, ``(TrainEngine, None)`` for both networks of an engine, read where the
    engine keeps them (its flat parameter and packed-weight blocks: no state_dict copy, no second module), or a pair of
    BaseNet2 modules (their flat blocks are laid side by side once per call)."""
    if isinstance(nets, tuple) and len(nets) == 2 and nets[1] is None and hasattr(nets[0], "params"):
        eng = nets[0]
        eng._ensure_packed(_lib.stream(eng.device))
        return eng.cshape, 2, eng.params, int(eng.params.shape[1]), eng.packed, int(eng.packed.shape[1]), False
    if isinstance(nets, (tuple, list)) and len(nets) == 2 and not hasattr(nets[0], "params"):
        bufs = [_net_buffers(m) for m in nets]
        (cs, f0, p0), (cs1, f1, p1) = bufs
        if tuple(getattr(cs, k) for k in "CHWK") + (cs.bands,) != tuple(getattr(cs1, k) for k in "CHWK") + (cs1.bands,):
            raise ValueError("the two networks differ in shape")
        return cs, 2, torch.stack((f0, f1)), f0.numel(), torch.stack((p0, p1)), p0.numel(), False
    cs, flat, packed = _net_buffers(nets)
    return cs, 1, flat, flat.numel(), packed, packed.numel(), True


def check_pixel_list(pix: torch.Tensor, rows: int, name: str = "pix") -> None:
    """Every entry of an int64 device list inside [0, rows): the kernels follow the list without a bounds check (the C
    call cannot look at device data without a synchronisation).  One synchronising min / max: where a list is SET UP."""
    if not (pix.is_cuda and pix.dtype == torch.int64 and pix.dim() == 1 and pix.is_contiguous() and pix.numel() >= 1):
        raise ValueError(f"{name}: need a non-empty contiguous int64 cuda vector")
    lo, hi = int(pix.min()), int(pix.max())
    if lo < 0 or hi >= rows:
        raise ValueError(f"{name}: entries span [{lo}, {hi}], valid are 0 .. {rows - 1}")


def _check_scene(cube, spectra, cs=None, whole: bool = False):
    """the scene contract: the cube, the spectra if any (``whole``: one row per scene pixel), both against the network shape"""
    if not (cube.is_cuda and cube.dtype == torch.float32 and cube.is_contiguous() and cube.dim() == 3):
        raise ValueError("cube: need contiguous float32 cuda tensor [rows, cols, C]")
    if spectra is not None and not (
            spectra.is_cuda and spectra.dtype == torch.float32 and spectra.is_contiguous() and spectra.dim() == 2
            and (not whole or spectra.shape[0] == cube.shape[0] * cube.shape[1])):
        raise ValueError(f"spectra: need contiguous float32 cuda tensor [{'rows * cols' if whole else '.'}, bands]")
    if cs is not None and (cube.shape[2] != cs.C or spectra.shape[1] != cs.bands):
        raise ValueError(f"cube has {cube.shape[2]} channels / spectra {spectra.shape[1]} bands, the network wants "
                         f"{cs.C} / {cs.bands}")
    if cs is not None and (cube.shape[0] < cs.H // 2 or cube.shape[1] < cs.W // 2):      # (the mirror index folds once)
        raise ValueError(f"scene of {cube.shape[0]} x {cube.shape[1]} pixels: a {cs.H} x {cs.W} window needs at least "
                         f"{cs.H // 2} x {cs.W // 2}")


class _Range(NamedTuple):
    """the feed of ``infer_cube``: pixels pixel0 .. pixel0 + n - 1 (n None: to the end of the scene)"""
    pixel0: int
    n: Optional[int]


class _List(NamedTuple):
    """the feed of ``infer_pixels``: a pixel list, its spectra rows, and whether their ranges are checked (synchronising)"""
    pix: torch.Tensor
    spec_rows: Optional[torch.Tensor]
    check: bool


def _check_feed(cube, spectra, feed) -> int:
    """the number of pixels of a feed that fits the scene"""
    total = cube.shape[0] * cube.shape[1]
    if isinstance(feed, _Range):
        n = total - feed.pixel0 if feed.n is None else int(feed.n)
        if feed.pixel0 < 0 or n < 1 or feed.pixel0 + n > total:
            raise ValueError("pixel range outside the scene")
        return n
    pix, spec_rows, check = feed
    if check:
        check_pixel_list(pix, total)
        if spec_rows is not None:
            check_pixel_list(spec_rows, spectra.shape[0], "spec_rows")
    n = pix.numel()
    if (spec_rows is not None and spec_rows.numel() != n) or (spec_rows is None and spectra.shape[0] < n):
        raise ValueError("spectra / spec_rows do not cover the pixel list")
    return n


def _same_shape(bufs):
    cs = bufs[0][0]
    for b in bufs:
        if (b[0].C, b[0].H, b[0].W, b[0].bands, b[0].K) != (cs.C, cs.H, cs.W, cs.bands, cs.K):
            raise ValueError("the networks differ in shape")
    return cs


def _first_max(z):
    """torch.max's rule, as in cmlpl_infer_cube: a NaN logit is the maximum, the first one wins"""
    nan = torch.isnan(z)
    return torch.where(nan.any(1), nan.int().argmax(1), z.argmax(1))


class _Forward:
    """The eval forward of one chunk of a feed (``_Range`` or ``_List``) for a clean call (key None) or a view key (sigma,
    seed, view, spatial element) when ``views``.  Asks the library once whether the window shape is fused, and owns what either way needs
    for chunks of up to ``self.chunk`` pixels: the
    fused calls' workspace (``nets``: the most networks one group holds), or -- windows of more than 256 pixels, the
    reference's 20 x 20 -- the by-patches buffers: ``chunk`` (4096 at the most) windows cut on the device
    (tools/hyper_tools.py:35-55,226-243; 393 MB at 20 x 20 x 60), their spectra, and the general eval forward's workspace.
    Nothing here synchronises; nothing is allocated after the constructor but the pieces of a list-fed chunk that does
    not cover its results and a clean list's gathered spectra rows by patches."""

    def __init__(self, lib, cs, nets: int, cube, spectra, feed, n: int, chunk: int, views: bool = False,
                 labels: bool = True):
        self.lib, self.cs, self.cube, self.spectra = lib, cs, cube, spectra
        self.pixel0 = pixel0 = feed.pixel0 if isinstance(feed, _Range) else None
        self.pix, self.spec_rows = (None, None) if pixel0 is not None else (feed.pix, feed.spec_rows)
        dev = cube.device
        chunk = max(8, min(int(chunk), n))
        if pixel0 is not None:
            if nets != 1:
                raise ValueError("the range-fed forward takes one network per call")
            self.name = "cmlpl_infer_cube_tta_sym" if views else "cmlpl_infer_cube"
            need = (lib.cmlpl_infer_tta_workspace_bytes if views else lib.cmlpl_infer_workspace_bytes)(C.byref(cs), chunk)
        else:
            self.name = "cmlpl_infer_pixels_tta_sym" if views else "cmlpl_infer_pixels"
            need = (lib.cmlpl_eval_tta_workspace_bytes if views else lib.cmlpl_eval_workspace_bytes)(C.byref(cs), nets, chunk)
        self.fused = need > 0
        if self.fused:
            self.own = None if labels else torch.empty(nets * chunk, dtype=torch.int64, device=dev)  # written, not used
        else:
            chunk = min(chunk, 4096)
            if cs.H != cs.W:
                raise _lib.CmlplError(self.name, -2)
            need = lib.cmlpl_workspace_bytes(C.byref(cs), 1, chunk, chunk)
            if need == 0:
                raise _lib.CmlplError("cmlpl_workspace_bytes", -2)
            cuts = 3 if views else 1          # (a view call cuts its clean block with cmlpl_extract_patches)
            if lib.cmlpl_patches_fit(cs.C, cs.H) & cuts != cuts:      # before anything is allocated or launched
                raise _lib.CmlplError("cmlpl_tta_patches_sym" if views else "cmlpl_extract_patches", -2)
            self.xp = torch.empty(chunk, cs.C, cs.H, cs.W, dtype=torch.float32, device=dev)
            self.x = torch.empty(chunk, cs.bands, dtype=torch.float32, device=dev) if views else None
            self.z = torch.empty(chunk, cs.K, dtype=torch.float32, device=dev)      # the logits nobody asked for
            self.feat = torch.empty(chunk, 1024, dtype=torch.float32, device=dev)
            if pixel0 is not None:
                self.pix = self.spec_rows = torch.arange(pixel0, pixel0 + n, dtype=torch.int64, device=dev)
        self.chunk = chunk
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def cut(self, o: int, m: int, key) -> None:
        """by patches: the windows and spectra rows of pixels [o, o + m) under ``key`` (cmlpl_extract_patches for a clean
        call, cmlpl_tta_patches for a view call, its clean block included)"""
        if self.fused:
            return
        cs, cube, sr = self.cs, self.cube, self.spec_rows
        rows, cols, _ = cube.shape
        st = _lib.stream(cube.device)
        if key is None:
            _lib.check("cmlpl_extract_patches", self.lib.cmlpl_extract_patches(
                cube.data_ptr(), rows, cols, cs.C, cs.H, self.pix.data_ptr() + 8 * o, m, self.xp.data_ptr(), st))
            if self.pixel0 is not None:
                self.x_ptr = self.spectra.data_ptr() + 4 * cs.bands * (self.pixel0 + o)
            else:
                self.rows_x = self.spectra[o:o + m] if sr is None else self.spectra[sr[o:o + m]].contiguous()
                self.x_ptr = self.rows_x.data_ptr()
        else:
            _lib.check("cmlpl_tta_patches_sym", self.lib.cmlpl_tta_patches_sym(
                cube.data_ptr(), rows, cols, cs.C, cs.H, self.pix.data_ptr() + 8 * o, m, self.xp.data_ptr(),
                self.spectra.data_ptr() + (0 if sr is not None else 4 * cs.bands * o),
                None if sr is None else sr.data_ptr() + 8 * o, cs.bands, self.x.data_ptr(), *key[:3], st, key[3]))
            self.x_ptr = self.x.data_ptr()

    def run(self, group, key, o: int, m: int, labels, logits, at: int) -> None:
        """the networks of ``group`` (what ``_nets_buffers`` returns) on pixels [o, o + m) under ``key``: their labels to
        columns at .. at + m - 1 of ``labels`` int64 [nets, L] and their logits to those of ``logits`` [nets, L, K];
        either may be None.  By patches ``cut(o, m, key)`` comes first."""
        cs, nn, flat, pstride, packed, kstride, _ = group
        cube, K = self.cube, cs.K
        rows, cols, _ = cube.shape
        st = _lib.stream(cube.device)
        view = () if key is None else key
        if not self.fused:
            flat2, packed2 = flat.view(nn, -1), packed.view(nn, -1)
            for j in range(nn):
                own_z = key is None or logits is None       # (a clean call goes through the scratch rows, a view call does not)
                z = self.z[:m] if own_z else logits[j, at:at + m]
                _lib.check("cmlpl_basenet2_fwd", self.lib.cmlpl_basenet2_fwd(
                    C.byref(cs), 1, m, flat2[j].data_ptr(), flat2[j].numel(), packed2[j].data_ptr(), self.xp.data_ptr(),
                    self.x_ptr, None, None, 0.0, 0, 0, 0, None, z.data_ptr(), self.feat.data_ptr(), self.ws.data_ptr(),
                    self.ws.numel(), st))
                if labels is not None:
                    labels[j, at:at + m] = _first_max(z)
                if own_z and logits is not None:
                    logits[j, at:at + m] = z
            return
        if labels is None:
            labels, at = self.own[:nn * m].view(nn, m), 0
        if self.pixel0 is not None:                           # (one network per call: its rows lie where they belong)
            _lib.check(self.name, getattr(self.lib, self.name)(
                C.byref(cs), flat.data_ptr(), packed.data_ptr(), cube.data_ptr(), rows, cols, self.spectra.data_ptr(),
                self.pixel0 + o, m, labels.data_ptr() + 8 * at, None if logits is None else logits.data_ptr() + 4 * K * at,
                self.ws.data_ptr(), self.ws.numel(), st, *view))
            return
        whole = labels.shape[1] == m      # (straight into the [nets][m] results; else through [nets][m] pieces)
        lab = labels if whole else torch.empty(nn, m, dtype=torch.int64, device=cube.device)
        lg = None if logits is None else (logits if whole else torch.empty(nn, m, K, dtype=torch.float32, device=cube.device))
        sr = self.spec_rows
        _lib.check(self.name, getattr(self.lib, self.name)(
            C.byref(cs), nn, flat.data_ptr(), pstride, packed.data_ptr(), kstride, cube.data_ptr(), rows, cols,
            self.spectra.data_ptr() + (0 if sr is not None else 4 * cs.bands * o),
            None if sr is None else sr.data_ptr() + 8 * o, self.pix.data_ptr() + 8 * o, m,
            lab.data_ptr(), _lib.ptr(lg), self.ws.data_ptr(), self.ws.numel(), st, *view))
        if not whole:
            labels[:, at:at + m] = lab
            if logits is not None:
                logits[:, at:at + m] = lg


def _predict(fwd: _Forward, groups, keys, n: int, labels=None, logits=None, buf=None, reduce=None) -> None:
    """THE chunk loop: per chunk of ``fwd.chunk`` pixels, per block (``keys``: None = a clean call, else a view key), per
    group of networks one forward.  Without ``reduce`` (one block, one group) the labels [nets, n] and logits
    [nets, n, K] are the results; with it every chunk's logits go to ``buf`` as [blocks, members, m, K] and
    ``reduce(z, o, m)`` follows."""
    M = sum(g[1] for g in groups)
    K, chunk = fwd.cs.K, fwd.chunk
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        z = None if reduce is None else buf[:len(keys) * M * m * K].view(len(keys), M, m, K)
        for vi, key in enumerate(keys):
            if key is not None:
                fwd.cut(o, m, key)                    # a view's windows are cut once and serve every network
            k = 0
            for g in groups:
                if key is None:
                    fwd.cut(o, m, None)               # a clean call cuts per group: each forward its own windows
                if reduce is None:
                    fwd.run(g, key, o, m, labels, logits, o)
                else:
                    fwd.run(g, key, o, m, None, z[vi, k:k + g[1]], 0)
                k += g[1]
        if reduce is not None:
            reduce(z, o, m)


def _infer(nets, cube, spectra, feed, chunk, want_logits: bool, key, out=None):
    """``infer_cube`` / ``infer_pixels`` or their view under ``key`` (cmlpl_amd.tta): the driver with one block, one group
    and no reduction: (labels, logits) or labels, new tensors or ``out``"""
    group = _nets_buffers(nets)
    cs, nn = group[0], group[1]
    _check_scene(cube, spectra, cs, whole=isinstance(feed, _Range))
    n = _check_feed(cube, spectra, feed)
    fwd = _Forward(_lib.load(), cs, nn, cube, spectra, feed, n, chunk, views=key is not None)
    dev = cube.device
    if out is None:
        labels = torch.empty(nn, n, dtype=torch.int64, device=dev)
        logits = torch.empty(nn, n, cs.K, dtype=torch.float32, device=dev) if want_logits else None
    else:
        labels, logits = out
        ok = labels.is_cuda and labels.dtype == torch.int64 and labels.is_contiguous() and tuple(labels.shape) == (n,)
        if want_logits:
            ok = ok and logits is not None and logits.is_cuda and logits.dtype == torch.float32 \
                and logits.is_contiguous() and tuple(logits.shape) == (n, cs.K)
        else:
            logits = None
        if not ok:
            raise ValueError("out: need contiguous cuda (int64 [n], float32 [n, K]) buffers")
    _predict(fwd, [group], [key], n, labels.view(nn, n), None if logits is None else logits.view(nn, n, cs.K))
    if out is None and group[6]:
        labels, logits = labels[0], (None if logits is None else logits[0])
    return (labels, logits) if want_logits else labels


@torch.no_grad()
def infer_cube(net, cube: torch.Tensor, spectra: torch.Tensor, pixel0: int = 0, n: Optional[int] = None,
               chunk: int = 65536, want_logits: bool = False, out=None):
    """argmax labels (int64 cuda [n]) of pixels pixel0 .. pixel0 + n - 1 (row-major; default: the whole scene), and the
    logits [n, K] when asked for.  Asynchronous.  Window shapes the fused per-sample forward does not take (more than 256
    window pixels: the reference's 20 x 20) go by patches (``_Forward``): same results, ``chunk`` pixels' windows in HBM
    at a time.  ``out``: (labels, logits) buffers that exist -- contiguous int64 [n] and float32 [n, K] (or None) -- are
    written instead of new tensors."""
    return _infer(net, cube, spectra, _Range(pixel0, n), chunk, want_logits, None, out)


@torch.no_grad()
def infer_pixels(nets, cube: torch.Tensor, spectra: torch.Tensor, pix: torch.Tensor, spec_rows: Optional[torch.Tensor] = None,
                 chunk: int = 65536, want_logits: bool = False, check: bool = True):
    """``infer_cube`` for a LIST of scene pixels (int64 cuda [n], row-major indices into ``cube``; any order, repeats
    allowed) and for both networks in one call (cmlpl_infer_pixels): what scoring a split needs -- its labelled pixels,
    not the scene.  Item i's spectrum is row ``spec_rows[i]`` of ``spectra``, or row i when ``spec_rows`` is None (the
    compact rows ``HSIDataSet.scene_arrays()`` hands over); ``spec_rows=pix`` with the whole scene's spectra is
    ``infer_cube``'s addressing.  ``nets``: see ``_nets_buffers``.  Returns labels int64 [n] for one network, [2, n] for
    two, and the logits ([n, K] / [2, n, K]) when asked for; equal to ``infer_cube`` at the same pixels bit for bit.
    ``check``: one synchronising range check of the lists (``Evaluator`` checks once, when a split is registered).
    Asynchronous otherwise."""
    return _infer(nets, cube, spectra, _List(pix, spec_rows, check), chunk, want_logits, None)
