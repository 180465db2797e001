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
        eng._ensure_packed(C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
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
    forward (cmlpl_basenet2_fwd).  Either way the scene stays in HBM as its cube; the 19.9 GB patch tensor never exists."""
    lib = _lib.load()
    cs = _lib.Shape(shape.C, shape.H, shape.W, shape.bands, shape.K)
    return shape.H == shape.W and lib.cmlpl_workspace_bytes(C.byref(cs), 1, 8, 8) > 0


@torch.no_grad()
def infer_cube(net, cube: torch.Tensor, spectra: torch.Tensor, pixel0: int = 0, n: Optional[int] = None,
               chunk: int = 65536, want_logits: bool = False, out=None):
    """argmax labels (int64 cuda [n]) of pixels pixel0 .. pixel0 + n - 1 (row-major; default: the whole scene), and the
    logits [n, K] when asked for.  Asynchronous.  Window shapes the fused per-sample forward does not take (more than 256
    window pixels: the reference's 20 x 20) go through ``_infer_cube_by_patches``: same results, ``chunk`` pixels' windows
    in HBM at a time.  ``out``: (labels, logits) buffers that exist -- contiguous int64 [n] and float32 [n, K] (or None)
    -- are written instead of new tensors (cmlpl_amd.ensemble fills one buffer with several networks' logits)."""
    if not (cube.is_cuda and cube.dtype == torch.float32 and cube.is_contiguous() and cube.dim() == 3):
        raise ValueError("cube: need contiguous float32 cuda tensor [rows, cols, C]")
    rows, cols, Cc = cube.shape
    if not (spectra.is_cuda and spectra.dtype == torch.float32 and spectra.is_contiguous() and spectra.dim() == 2
            and spectra.shape[0] == rows * cols):
        raise ValueError("spectra: need contiguous float32 cuda tensor [rows * cols, bands]")
    cs, flat, packed = _net_buffers(net)
    if Cc != cs.C or spectra.shape[1] != cs.bands:
        raise ValueError(f"cube has {Cc} channels / spectra {spectra.shape[1]} bands, the network wants {cs.C} / {cs.bands}")
    n = rows * cols - pixel0 if n is None else int(n)
    if pixel0 < 0 or n < 1 or pixel0 + n > rows * cols:
        raise ValueError("pixel range outside the scene")
    lib = _lib.load()
    dev = cube.device
    if out is None:
        labels = torch.empty(n, dtype=torch.int64, device=dev)
        logits = torch.empty(n, cs.K, dtype=torch.float32, device=dev) if want_logits else None
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
    chunk = max(8, min(int(chunk), n))
    need = lib.cmlpl_infer_workspace_bytes(C.byref(cs), chunk)
    if need == 0:                                           # not a window the fused per-sample forward takes
        _infer_cube_by_patches(lib, cs, flat, packed, cube, spectra, pixel0, n, min(chunk, 4096), labels, logits)
        return (labels, logits) if want_logits else labels
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        _lib.check("cmlpl_infer_cube", lib.cmlpl_infer_cube(
            C.byref(cs), flat.data_ptr(), packed.data_ptr(), cube.data_ptr(), rows, cols, spectra.data_ptr(),
            pixel0 + o, m, labels.data_ptr() + 8 * o, None if logits is None else logits.data_ptr() + 4 * cs.K * o,
            ws.data_ptr(), ws.numel(), st))
    return (labels, logits) if want_logits else labels


def _infer_cube_by_patches(lib, cs, flat, packed, cube, spectra, pixel0, n, chunk, labels, logits):
    """``chunk`` pixels at a time: their windows cut from the cube on the device (cmlpl_extract_patches: mirror index,
    tools/hyper_tools.py:35-55,226-243), the general eval forward on them (cmlpl_basenet2_fwd, one network, no dropout),
    argmax (first maximum, NaN first: torch.max's rule, as in cmlpl_infer_cube).  One patch buffer of chunk x C x w x w
    floats (393 MB at 4096 pixels of 20 x 20 x 60) is re-used; nothing leaves the device."""
    if cs.H != cs.W:
        raise _lib.CmlplError("cmlpl_infer_cube", -2)
    dev = cube.device
    rows, cols, _ = cube.shape
    need = lib.cmlpl_workspace_bytes(C.byref(cs), 1, chunk, chunk)
    if need == 0:
        raise _lib.CmlplError("cmlpl_workspace_bytes", -2)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    xp = torch.empty(chunk, cs.C, cs.H, cs.W, dtype=torch.float32, device=dev)
    z = torch.empty(chunk, cs.K, dtype=torch.float32, device=dev)
    feat = torch.empty(chunk, 1024, dtype=torch.float32, device=dev)
    idx = torch.arange(pixel0, pixel0 + n, dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        _lib.check("cmlpl_extract_patches", lib.cmlpl_extract_patches(
            cube.data_ptr(), rows, cols, cs.C, cs.H, idx.data_ptr() + 8 * o, m, xp.data_ptr(), st))
        _lib.check("cmlpl_basenet2_fwd", lib.cmlpl_basenet2_fwd(
            C.byref(cs), 1, m, flat.data_ptr(), flat.numel(), packed.data_ptr(), xp.data_ptr(),
            spectra.data_ptr() + 4 * cs.bands * (pixel0 + o), None, None, 0.0, 0, 0, 0, None,
            z.data_ptr(), feat.data_ptr(), ws.data_ptr(), ws.numel(), st))
        zz = z[:m]
        nan = torch.isnan(zz)                                   # torch.max: a NaN logit is the maximum, the first one wins
        lab = torch.where(nan.any(1), nan.int().argmax(1), zz.argmax(1))
        labels[o:o + m] = lab
        if logits is not None:
            logits[o:o + m] = zz


def _nets_buffers(nets):
    """(shape struct, n networks, parameters, parameter stride, packed weights, packed stride, squeeze) of what
    ``infer_pixels`` was given: ONE network as ``_net_buffers`` takes it (a BaseNet2 module or (TrainEngine, index)) --
    then the results carry no network dimension --, ``(TrainEngine, None)`` for both networks of an engine, read where the
    engine keeps them (its flat parameter and packed-weight blocks: no state_dict copy, no second module), or a pair of
    BaseNet2 modules (their flat blocks are laid side by side once per call)."""
    if isinstance(nets, tuple) and len(nets) == 2 and nets[1] is None and hasattr(nets[0], "params"):
        eng = nets[0]
        eng._ensure_packed(C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
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


def _infer_pixels_into(lib, cs, nn, flat, pstride, packed, kstride, cube, spectra, spec_rows, pix, labels, logits, ws,
                       chunk):
    """the launches of ``infer_pixels`` into buffers that exist: labels [nn][n] int64, logits [nn][n][K] or None, ws the
    workspace of one chunk (cmlpl_eval_workspace_bytes; None: the window shape goes by patches).  No allocation when the
    list fits one chunk; no synchronisation."""
    n = pix.numel()
    rows, cols, _ = cube.shape
    if ws is None:
        _infer_pixels_by_patches(lib, cs, nn, flat, packed, cube, spectra, spec_rows, pix, min(chunk, 4096), labels, logits)
        return
    st = C.c_void_p(torch.cuda.current_stream(cube.device).cuda_stream)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        whole = m == n                    # (one call: straight into the [nets][n] results; else through [nets][m] pieces)
        lab = labels if whole else torch.empty(nn, m, dtype=torch.int64, device=cube.device)
        lg = None if logits is None else (logits if whole else torch.empty(nn, m, cs.K, dtype=torch.float32, device=cube.device))
        _lib.check("cmlpl_infer_pixels", lib.cmlpl_infer_pixels(
            C.byref(cs), nn, flat.data_ptr(), pstride, packed.data_ptr(), kstride, cube.data_ptr(), rows, cols,
            spectra.data_ptr() + (0 if spec_rows is not None else 4 * cs.bands * o),
            None if spec_rows is None else spec_rows.data_ptr() + 8 * o, pix.data_ptr() + 8 * o, m,
            lab.data_ptr(), None if lg is None else lg.data_ptr(), ws.data_ptr(), ws.numel(), st))
        if not whole:
            labels[:, o:o + m] = lab
            if logits is not None:
                logits[:, o:o + m] = lg


def _infer_pixels_by_patches(lib, cs, nn, flat, packed, cube, spectra, spec_rows, pix, chunk, labels, logits):
    """``_infer_cube_by_patches`` for a list: cmlpl_extract_patches takes the list as it is, each chunk's windows are cut
    ONCE and serve every network (the general eval forward, one network per call, as ``infer_cube`` runs it)."""
    if cs.H != cs.W:
        raise _lib.CmlplError("cmlpl_infer_pixels", -2)
    dev = cube.device
    rows, cols, _ = cube.shape
    n = pix.numel()
    need = lib.cmlpl_workspace_bytes(C.byref(cs), 1, chunk, chunk)
    if need == 0:
        raise _lib.CmlplError("cmlpl_workspace_bytes", -2)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    xp = torch.empty(chunk, cs.C, cs.H, cs.W, dtype=torch.float32, device=dev)
    z = torch.empty(chunk, cs.K, dtype=torch.float32, device=dev)
    feat = torch.empty(chunk, 1024, dtype=torch.float32, device=dev)
    flat2, packed2 = flat.view(nn, -1), packed.view(nn, -1)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        _lib.check("cmlpl_extract_patches", lib.cmlpl_extract_patches(
            cube.data_ptr(), rows, cols, cs.C, cs.H, pix.data_ptr() + 8 * o, m, xp.data_ptr(), st))
        x = spectra[o:o + m] if spec_rows is None else spectra[spec_rows[o:o + m]].contiguous()
        for k in range(nn):
            _lib.check("cmlpl_basenet2_fwd", lib.cmlpl_basenet2_fwd(
                C.byref(cs), 1, m, flat2[k].data_ptr(), flat2[k].numel(), packed2[k].data_ptr(), xp.data_ptr(),
                x.data_ptr(), None, None, 0.0, 0, 0, 0, None, z.data_ptr(), feat.data_ptr(), ws.data_ptr(), ws.numel(), st))
            zz = z[:m]
            nan = torch.isnan(zz)                               # torch.max's rule, as in _infer_cube_by_patches
            labels[k, o:o + m] = torch.where(nan.any(1), nan.int().argmax(1), zz.argmax(1))
            if logits is not None:
                logits[k, o:o + m] = zz


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
    if not (cube.is_cuda and cube.dtype == torch.float32 and cube.is_contiguous() and cube.dim() == 3):
        raise ValueError("cube: need contiguous float32 cuda tensor [rows, cols, C]")
    rows, cols, Cc = cube.shape
    if not (spectra.is_cuda and spectra.dtype == torch.float32 and spectra.is_contiguous() and spectra.dim() == 2):
        raise ValueError("spectra: need contiguous float32 cuda tensor [., bands]")
    cs, nn, flat, pstride, packed, kstride, squeeze = _nets_buffers(nets)
    if Cc != cs.C or spectra.shape[1] != cs.bands:
        raise ValueError(f"cube has {Cc} channels / spectra {spectra.shape[1]} bands, the network wants {cs.C} / {cs.bands}")
    if check:
        check_pixel_list(pix, rows * cols)
        if spec_rows is not None:
            check_pixel_list(spec_rows, spectra.shape[0], "spec_rows")
    n = pix.numel()
    if (spec_rows is not None and spec_rows.numel() != n) or (spec_rows is None and spectra.shape[0] < n):
        raise ValueError("spectra / spec_rows do not cover the pixel list")
    lib = _lib.load()
    dev = cube.device
    labels = torch.empty(nn, n, dtype=torch.int64, device=dev)
    logits = torch.empty(nn, n, cs.K, dtype=torch.float32, device=dev) if want_logits else None
    chunk = max(8, min(int(chunk), n))
    need = lib.cmlpl_eval_workspace_bytes(C.byref(cs), nn, chunk)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    _infer_pixels_into(lib, cs, nn, flat, pstride, packed, kstride, cube, spectra, spec_rows, pix, labels, logits, ws, chunk)
    if squeeze:
        labels, logits = labels[0], (None if logits is None else logits[0])
    return (labels, logits) if want_logits else labels
