"""Test-time augmentation: a prediction from several noisy VIEWS of every pixel -- x + sigma N(0,1) on window and
spectrum, the kind of input the networks were trained on (``train.py --m``, which the reference parses and never uses) --
averaged over views and networks on the device.

A view is defined in ``include/cmlpl.h`` ("THE DEFINITION OF A VIEW"): view ``t`` of scene pixel ``P`` under
``(seed, sigma)`` is a property of ``(seed, t, P)`` alone -- every network scores the same views, whatever the chunk, the
list order or the kind of launch.  The fused cube-fed forward adds the noise while it stages its slab
(``cmlpl_infer_cube_tta`` / ``cmlpl_infer_pixels_tta``: no window tensor in HBM); window shapes it does not take go by
patches (``cmlpl_tta_patches`` + the general eval forward), a few thousand pixels at a time.  Per chunk every
member x view forward writes into one reused logits buffer [blocks, members, chunk, K] and one ``cmlpl_ensemble_views``
launch follows: ``p = sum_m sum_v w_m / V softmax(z_mv)``, label / confidence / entropy as in ``cmlpl_amd.ensemble``,
``disagree`` = the number of (member, view) blocks whose own label differs.  Nothing here synchronises."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from .ensemble import EnsembleResult, _alloc, _groups, _weights
from .infer import _nets_buffers, check_pixel_list

MAX_BLOCKS = 64          # members x (views + clean), cmlpl_ensemble_views


class TTA(NamedTuple):
    """``views`` noisy views at ``sigma`` under ``seed``; ``clean``: the plain forward's logits are one more block, in front"""
    views: int
    sigma: float
    seed: int = 1088
    clean: bool = True

    def blocks(self):
        """the views a member scores, in the order of their blocks: None = the clean window, else the view index"""
        v = int(self.views)
        if v < 0 or (v == 0 and not self.clean):
            raise ValueError("TTA: need at least one view (views >= 1, or views == 0 with clean=True)")
        if not (float(self.sigma) >= 0.0) or float(self.sigma) == float("inf"):
            raise ValueError("TTA: sigma must be finite and >= 0")
        if not 0 <= int(self.seed) < 2 ** 64:
            raise ValueError("TTA: seed must fit 64 bits")
        return ([None] if self.clean else []) + list(range(v))


def _check_blocks(tta: TTA, members: int):
    blocks = tta.blocks()
    if members * len(blocks) > MAX_BLOCKS:
        raise ValueError(f"TTA: {members} members x {len(blocks)} blocks, cmlpl_ensemble_views takes up to {MAX_BLOCKS}")
    return blocks


def _key(tta: TTA, t):
    """(sigma, seed, view) of block ``t``; the clean block is sigma 0 (the clean forward's launches and bytes)"""
    return (C.c_float(0.0 if t is None else float(tta.sigma)), C.c_uint64(int(tta.seed)), C.c_uint32(0 if t is None else int(t)))


def _check_scene(cube, spectra, cs):
    if not (cube.is_cuda and cube.dtype == torch.float32 and cube.is_contiguous() and cube.dim() == 3):
        raise ValueError("cube: need contiguous float32 cuda tensor [rows, cols, C]")
    if not (spectra.is_cuda and spectra.dtype == torch.float32 and spectra.is_contiguous() and spectra.dim() == 2):
        raise ValueError("spectra: need contiguous float32 cuda tensor [., bands]")
    if cs is not None and (cube.shape[2] != cs.C or spectra.shape[1] != cs.bands):
        raise ValueError(f"cube has {cube.shape[2]} channels / spectra {spectra.shape[1]} bands, the network wants "
                         f"{cs.C} / {cs.bands}")


def _same_shape(bufs):
    cs = bufs[0][0]
    for b in bufs:
        if (b[0].C, b[0].H, b[0].W, b[0].bands, b[0].K) != (cs.C, cs.H, cs.W, cs.bands, cs.K):
            raise ValueError("the networks differ in shape")
    return cs


class _Patches:
    """the by-patches path's buffers for chunks of up to ``chunk`` pixels: one view's windows and spectra serve every member"""

    def __init__(self, lib, cs, chunk, dev):
        if cs.H != cs.W:
            raise _lib.CmlplError("cmlpl_tta_patches", -2)
        need = lib.cmlpl_workspace_bytes(C.byref(cs), 1, chunk, chunk)
        if need == 0:
            raise _lib.CmlplError("cmlpl_workspace_bytes", -2)
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.xp = torch.empty(chunk, cs.C, cs.H, cs.W, dtype=torch.float32, device=dev)
        self.x = torch.empty(chunk, cs.bands, dtype=torch.float32, device=dev)
        self.feat = torch.empty(chunk, 1024, dtype=torch.float32, device=dev)

    def cut(self, lib, cs, cube, spectra_ptr, spec_rows_ptr, pix_ptr, m, key, st):
        rows, cols, _ = cube.shape
        _lib.check("cmlpl_tta_patches", lib.cmlpl_tta_patches(
            cube.data_ptr(), rows, cols, cs.C, cs.H, pix_ptr, m, self.xp.data_ptr(), spectra_ptr, spec_rows_ptr, cs.bands,
            self.x.data_ptr(), *key, st))

    def forward(self, lib, cs, flat, packed, m, z_ptr, st):
        _lib.check("cmlpl_basenet2_fwd", lib.cmlpl_basenet2_fwd(
            C.byref(cs), 1, m, flat.data_ptr(), flat.numel(), packed.data_ptr(), self.xp.data_ptr(), self.x.data_ptr(),
            None, None, 0.0, 0, 0, 0, None, z_ptr, self.feat.data_ptr(), self.ws.data_ptr(), self.ws.numel(), st))


def _reduce(lib, z, M, V, m, K, cw, res: EnsembleResult, o, st):
    """one cmlpl_ensemble_views over the chunk's blocks z [V, M, m, K]; results to rows o .. o + m - 1"""
    at = lambda t, size: None if t is None else t.data_ptr() + size * o
    _lib.check("cmlpl_ensemble_views", lib.cmlpl_ensemble_views(
        z.data_ptr(), M, V, m * K, M * m * K, cw, m, K, at(res.labels, 8), at(res.probs, 4 * K), at(res.conf, 4),
        at(res.entropy, 4), at(res.disagree, 4), st))


@torch.no_grad()
def tta_cube(nets, cube: torch.Tensor, spectra: torch.Tensor, tta: TTA, pixel0: int = 0, n: Optional[int] = None,
             chunk: int = 65536, weights: Optional[Sequence[float]] = None, probs: bool = False, conf: bool = False,
             entropy: bool = False, disagree: bool = False) -> EnsembleResult:
    """``ensemble_cube`` over the views of ``tta``: pixels pixel0 .. pixel0 + n - 1 of the scene (default: all of it),
    ``nets`` as ``cmlpl_amd.ensemble._groups`` takes them (1..4 members).  Every window shape ``infer_supported`` accepts.
    Asynchronous."""
    groups, M = _groups(nets)
    members = []
    for e, k in groups:
        members += [(e[0], 0), (e[0], 1)] if k == 2 else [e]
    blocks = _check_blocks(tta, M)
    bufs = [_nets_buffers(e) for e in members]              # (cs, 1, flat, ., packed, ., .)
    cs = _same_shape(bufs)
    _check_scene(cube, spectra, cs)
    rows, cols, _ = cube.shape
    if spectra.shape[0] != rows * cols:
        raise ValueError("spectra: need one row per scene pixel")
    n = rows * cols - pixel0 if n is None else int(n)
    if pixel0 < 0 or n < 1 or pixel0 + n > rows * cols:
        raise ValueError("pixel range outside the scene")
    K, V = cs.K, len(blocks)
    cw = _weights(weights, M)
    lib, dev = _lib.load(), cube.device
    chunk = max(8, min(int(chunk), n))
    fused = lib.cmlpl_infer_tta_workspace_bytes(C.byref(cs), chunk) > 0
    if not fused:
        chunk = min(chunk, 4096)
    res = _alloc(n, K, dev, probs, conf, entropy, disagree)
    buf = torch.empty(V * M * chunk * K, dtype=torch.float32, device=dev)
    own = torch.empty(chunk, dtype=torch.int64, device=dev)            # a block's own argmax: written, not used
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if fused:
        ws = torch.empty(lib.cmlpl_infer_tta_workspace_bytes(C.byref(cs), chunk), dtype=torch.uint8, device=dev)
    else:
        pt = _Patches(lib, cs, chunk, dev)
        idx = torch.arange(pixel0, pixel0 + n, dtype=torch.int64, device=dev)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        z = buf[:V * M * m * K].view(V, M, m, K)
        for vi, t in enumerate(blocks):
            key = _key(tta, t)
            if not fused:
                pt.cut(lib, cs, cube, spectra.data_ptr(), idx.data_ptr() + 8 * o, idx.data_ptr() + 8 * o, m, key, st)
            for k, b in enumerate(bufs):
                if fused:
                    _lib.check("cmlpl_infer_cube_tta", lib.cmlpl_infer_cube_tta(
                        C.byref(cs), b[2].data_ptr(), b[4].data_ptr(), cube.data_ptr(), rows, cols, spectra.data_ptr(),
                        pixel0 + o, m, own.data_ptr(), z[vi, k].data_ptr(), ws.data_ptr(), ws.numel(), st, *key))
                else:
                    pt.forward(lib, cs, b[2], b[4], m, z[vi, k].data_ptr(), st)
        _reduce(lib, z, M, V, m, K, cw, res, o, st)
    return res


@torch.no_grad()
def tta_pixels(nets, cube: torch.Tensor, spectra: torch.Tensor, pix: torch.Tensor, tta: TTA,
               spec_rows: Optional[torch.Tensor] = None, chunk: int = 65536, weights: Optional[Sequence[float]] = None,
               probs: bool = False, conf: bool = False, entropy: bool = False, disagree: bool = False,
               check: bool = True) -> EnsembleResult:
    """``tta_cube`` for a LIST of scene pixels, through the list-fed forward (``ensemble_pixels``' addressing: item i's
    spectrum is row ``spec_rows[i]`` of ``spectra``, or row i; its VIEW is that of scene pixel ``pix[i]`` either way).
    ``(engine, None)`` scores both networks in one forward launch chain per view.  ``check``: one synchronising range
    check of the lists.  Asynchronous otherwise."""
    groups, M = _groups(nets)
    blocks = _check_blocks(tta, M)
    bufs = [_nets_buffers(e) for e, _ in groups]            # (cs, nn, flat, pstride, packed, kstride, .)
    cs = _same_shape(bufs)
    _check_scene(cube, spectra, cs)
    rows, cols, _ = cube.shape
    if check:
        check_pixel_list(pix, rows * cols)
        if spec_rows is not None:
            check_pixel_list(spec_rows, spectra.shape[0], "spec_rows")
    n = pix.numel()
    if (spec_rows is not None and spec_rows.numel() != n) or (spec_rows is None and spectra.shape[0] < n):
        raise ValueError("spectra / spec_rows do not cover the pixel list")
    K, V = cs.K, len(blocks)
    cw = _weights(weights, M)
    lib, dev = _lib.load(), cube.device
    chunk = max(8, min(int(chunk), n))
    needs = [lib.cmlpl_eval_tta_workspace_bytes(C.byref(b[0]), b[1], chunk) for b in bufs]
    fused = min(needs) > 0
    if not fused:
        chunk = min(chunk, 4096)
    res = _alloc(n, K, dev, probs, conf, entropy, disagree)
    buf = torch.empty(V * M * chunk * K, dtype=torch.float32, device=dev)
    own = torch.empty(2 * chunk, dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if fused:
        ws = torch.empty(max(needs), dtype=torch.uint8, device=dev)
    else:
        pt = _Patches(lib, cs, chunk, dev)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        z = buf[:V * M * m * K].view(V, M, m, K)
        sp_ptr = spectra.data_ptr() + (0 if spec_rows is not None else 4 * cs.bands * o)
        sr_ptr = None if spec_rows is None else spec_rows.data_ptr() + 8 * o
        for vi, t in enumerate(blocks):
            key = _key(tta, t)
            if not fused:
                pt.cut(lib, cs, cube, sp_ptr, sr_ptr, pix.data_ptr() + 8 * o, m, key, st)
            k = 0
            for bcs, nn, flat, pstride, packed, kstride, _ in bufs:
                if fused:
                    _lib.check("cmlpl_infer_pixels_tta", lib.cmlpl_infer_pixels_tta(
                        C.byref(bcs), nn, flat.data_ptr(), pstride, packed.data_ptr(), kstride, cube.data_ptr(), rows, cols,
                        sp_ptr, sr_ptr, pix.data_ptr() + 8 * o, m, own.data_ptr(), z[vi, k].data_ptr(), ws.data_ptr(),
                        ws.numel(), st, *key))
                else:
                    f2, p2 = flat.view(nn, -1), packed.view(nn, -1)
                    for j in range(nn):
                        pt.forward(lib, bcs, f2[j], p2[j], m, z[vi, k + j].data_ptr(), st)
                k += nn
        _reduce(lib, z, M, V, m, K, cw, res, o, st)
    return res


@torch.no_grad()
def views_of(cube: torch.Tensor, spectra: Optional[torch.Tensor], pix: torch.Tensor, window: int, tta: TTA, t: int,
             spec_rows: Optional[torch.Tensor] = None):
    """view ``t`` of the scene pixels ``pix`` (int64 cuda [n]) as tensors: the windows [n, C, window, window] and -- when
    ``spectra`` is given -- the spectra [n, bands] (row ``spec_rows[i]``, or row ``pix[i]`` of the whole scene's spectra
    when ``spec_rows`` is None) with the view's noise: what the fused forward forms in registers (``cmlpl_tta_patches``).
    ``t=None``: the clean windows and rows.  Asynchronous."""
    if not (cube.is_cuda and cube.dtype == torch.float32 and cube.is_contiguous() and cube.dim() == 3):
        raise ValueError("cube: need contiguous float32 cuda tensor [rows, cols, C]")
    if not (pix.is_cuda and pix.dtype == torch.int64 and pix.dim() == 1 and pix.is_contiguous() and pix.numel() >= 1):
        raise ValueError("pix: need a non-empty contiguous int64 cuda vector")
    tta.blocks()
    rows, cols, Cc = cube.shape
    n, dev = pix.numel(), cube.device
    xp = torch.empty(n, Cc, window, window, dtype=torch.float32, device=dev)
    x = None
    sr = pix if spec_rows is None else spec_rows
    if spectra is not None:
        if not (spectra.is_cuda and spectra.dtype == torch.float32 and spectra.is_contiguous() and spectra.dim() == 2):
            raise ValueError("spectra: need contiguous float32 cuda tensor [., bands]")
        x = torch.empty(n, spectra.shape[1], dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check("cmlpl_tta_patches", _lib.load().cmlpl_tta_patches(
        cube.data_ptr(), rows, cols, Cc, int(window), pix.data_ptr(), n, xp.data_ptr(),
        None if spectra is None else spectra.data_ptr(), None if spectra is None else sr.data_ptr(),
        0 if spectra is None else spectra.shape[1], None if x is None else x.data_ptr(), *_key(tta, t), st))
    return xp, x


@torch.no_grad()
def ensemble_views_logits(logits: torch.Tensor, weights: Optional[Sequence[float]] = None, probs: bool = False,
                          conf: bool = False, entropy: bool = False, disagree: bool = False) -> EnsembleResult:
    """``cmlpl_ensemble_views`` on logits that exist: [M, V, n, K] float32 cuda, contiguous in its last two dimensions, the
    blocks anywhere as long as they do not overlap (the library checks the two strides).  One launch, no synchronisation."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4):
        raise ValueError("logits: need a float32 cuda tensor [M, V, n, K]")
    M, V, n, K = logits.shape
    if logits.stride(3) != 1 or logits.stride(2) != K:
        raise ValueError("logits: the last two dimensions must be contiguous")
    if not 1 <= M * V <= MAX_BLOCKS:
        raise ValueError(f"logits: {M} x {V} blocks, cmlpl_ensemble_views takes 1 .. {MAX_BLOCKS}")
    res = _alloc(n, K, logits.device, probs, conf, entropy, disagree)
    st = C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)
    _lib.check("cmlpl_ensemble_views", _lib.load().cmlpl_ensemble_views(
        logits.data_ptr(), M, V, logits.stride(0), logits.stride(1), _weights(weights, M), n, K, res.labels.data_ptr(),
        None if res.probs is None else res.probs.data_ptr(), None if res.conf is None else res.conf.data_ptr(),
        None if res.entropy is None else res.entropy.data_ptr(), None if res.disagree is None else res.disagree.data_ptr(),
        st))
    return res


@torch.no_grad()
def infer_cube_view(net, cube: torch.Tensor, spectra: torch.Tensor, tta: TTA, t, pixel0: int = 0,
                    n: Optional[int] = None, chunk: int = 65536):
    """``infer_cube(want_logits=True)`` of ONE network on view ``t`` (None: the clean window) of pixels pixel0 ..
    pixel0 + n - 1: (labels int64 [n], logits [n, K]) -- one block of what ``tta_cube`` reduces.  Asynchronous."""
    cs, _, flat, _, packed, _, _ = _nets_buffers(net)
    _check_scene(cube, spectra, cs)
    rows, cols, _ = cube.shape
    if spectra.shape[0] != rows * cols:
        raise ValueError("spectra: need one row per scene pixel")
    n = rows * cols - pixel0 if n is None else int(n)
    if pixel0 < 0 or n < 1 or pixel0 + n > rows * cols:
        raise ValueError("pixel range outside the scene")
    tta.blocks()
    lib, dev = _lib.load(), cube.device
    key = _key(tta, t)
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    logits = torch.empty(n, cs.K, dtype=torch.float32, device=dev)
    chunk = max(8, min(int(chunk), n))
    need = lib.cmlpl_infer_tta_workspace_bytes(C.byref(cs), chunk)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        chunk = min(chunk, 4096)
        pt = _Patches(lib, cs, chunk, dev)
        idx = torch.arange(pixel0, pixel0 + n, dtype=torch.int64, device=dev)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        if need:
            _lib.check("cmlpl_infer_cube_tta", lib.cmlpl_infer_cube_tta(
                C.byref(cs), flat.data_ptr(), packed.data_ptr(), cube.data_ptr(), rows, cols, spectra.data_ptr(), pixel0 + o, m,
                labels.data_ptr() + 8 * o, logits.data_ptr() + 4 * cs.K * o, ws.data_ptr(), ws.numel(), st, *key))
        else:
            pt.cut(lib, cs, cube, spectra.data_ptr(), idx.data_ptr() + 8 * o, idx.data_ptr() + 8 * o, m, key, st)
            pt.forward(lib, cs, flat, packed, m, logits.data_ptr() + 4 * cs.K * o, st)
            zz = logits[o:o + m]
            nan = torch.isnan(zz)                               # torch.max's rule, as in cmlpl_infer_cube
            labels[o:o + m] = torch.where(nan.any(1), nan.int().argmax(1), zz.argmax(1))
    return labels, logits


@torch.no_grad()
def infer_pixels_view(nets, cube: torch.Tensor, spectra: torch.Tensor, pix: torch.Tensor, tta: TTA, t,
                      spec_rows: Optional[torch.Tensor] = None, chunk: int = 65536, check: bool = True):
    """``infer_pixels(want_logits=True)`` on view ``t`` (None: clean) of a pixel list, ``nets`` as ``infer_pixels`` takes
    them: (labels [n] or [2, n], logits [n, K] or [2, n, K]); fused window shapes only.  Asynchronous but for ``check``."""
    cs, nn, flat, pstride, packed, kstride, squeeze = _nets_buffers(nets)
    _check_scene(cube, spectra, cs)
    rows, cols, _ = cube.shape
    if check:
        check_pixel_list(pix, rows * cols)
        if spec_rows is not None:
            check_pixel_list(spec_rows, spectra.shape[0], "spec_rows")
    n = pix.numel()
    if (spec_rows is not None and spec_rows.numel() != n) or (spec_rows is None and spectra.shape[0] < n):
        raise ValueError("spectra / spec_rows do not cover the pixel list")
    tta.blocks()
    lib, dev = _lib.load(), cube.device
    key = _key(tta, t)
    chunk = max(8, min(int(chunk), n))
    need = lib.cmlpl_eval_tta_workspace_bytes(C.byref(cs), nn, chunk)
    if need == 0:
        raise _lib.CmlplError("cmlpl_infer_pixels_tta", -2)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    labels = torch.empty(nn, n, dtype=torch.int64, device=dev)
    logits = torch.empty(nn, n, cs.K, dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        whole = m == n
        lab = labels if whole else torch.empty(nn, m, dtype=torch.int64, device=dev)
        lg = logits if whole else torch.empty(nn, m, cs.K, dtype=torch.float32, device=dev)
        _lib.check("cmlpl_infer_pixels_tta", lib.cmlpl_infer_pixels_tta(
            C.byref(cs), nn, flat.data_ptr(), pstride, packed.data_ptr(), kstride, cube.data_ptr(), rows, cols,
            spectra.data_ptr() + (0 if spec_rows is not None else 4 * cs.bands * o),
            None if spec_rows is None else spec_rows.data_ptr() + 8 * o, pix.data_ptr() + 8 * o, m,
            lab.data_ptr(), lg.data_ptr(), ws.data_ptr(), ws.numel(), st, *key))
        if not whole:
            labels[:, o:o + m] = lab
            logits[:, o:o + m] = lg
    if squeeze:
        labels, logits = labels[0], logits[0]
    return labels, logits
