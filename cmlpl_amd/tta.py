"""Test-time augmentation: a prediction from several noisy VIEWS of every pixel -- x + sigma N(0,1) on window and
spectrum, the kind of input the networks were trained on (``train.py --m``, which the reference parses and never uses) --
averaged over views and networks on the device.

A view is defined in ``include/cmlpl.h`` ("THE DEFINITION OF A VIEW"): view ``t`` of scene pixel ``P`` under
``(seed, sigma)`` is a property of ``(seed, t, P)`` alone -- every network scores the same views, whatever the chunk, the
list order or the kind of launch.  The fused cube-fed forward adds the noise while it stages its slab
(``cmlpl_infer_cube_tta`` / ``cmlpl_infer_pixels_tta``: no window tensor in HBM); window shapes it does not take go by
patches (``cmlpl_tta_patches`` + the general eval forward), a few thousand pixels at a time.
A view may also carry a SPATIAL element -- a flip or a rotation of the window's own index grid (``include/cmlpl.h``, "THE
DEFINITION OF A SPATIAL ELEMENT"; ``TTA(spatial="flips" | "d4")``, what ``TrainEngine(aug_spatial=...)`` trains on): the
same gathers with the window index remapped in front of the source address, the noise keyed by the output position.  ``tta_*`` are
``cmlpl_amd.ensemble._ensemble`` on the blocks of a ``TTA``: per chunk every member x view forward writes into one reused
logits buffer [blocks, members, chunk, K] and one ``cmlpl_ensemble_views`` launch follows:
``p = sum_m sum_v w_m / V softmax(z_mv)``, label / confidence / entropy as in ``cmlpl_amd.ensemble``, ``disagree`` = the
number of (member, view) blocks whose own label differs.  Nothing here synchronises."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from .ensemble import EnsembleResult, _alloc, _ensemble, _reduce, _weights
from .infer import _check_scene, _infer, _List, _Range

MAX_BLOCKS = 64          # members x (views + clean), cmlpl_ensemble_views


class TTA(NamedTuple):
    """``views`` noisy views at ``sigma`` under ``seed``; ``clean``: the plain forward's logits are one more block, in front;
    ``spatial``: the views walk the spatial elements of that mode ("none", "flips": 4, "d4": 8), view ``t`` takes element
    ``(t + (1 if clean else 0)) mod S`` -- ``TTA(7, 0.0, clean=True, spatial="d4")`` is the plain D4 orbit, each element once"""
    views: int
    sigma: float
    seed: int = 1088
    clean: bool = True
    spatial: str = "none"

    def pairs(self):
        """the blocks a member scores, in their order, as (t, g): the view index (None = the clean window) and its spatial
        element (0 = the window as it is)"""
        S = _lib.spatial_elements(self.spatial)
        c = 1 if self.clean else 0
        return [(t, 0 if t is None else (t + c) % S) for t in self._views()]

    def blocks(self):
        """the blocks a member scores, in their order: with ``spatial="none"`` the view indices (None = the clean window),
        else the (t, g) of ``pairs()``"""
        return self._views() if self.spatial == "none" else self.pairs()

    def _views(self):
        v = int(self.views)
        if v < 0 or (v == 0 and not self.clean):
            raise ValueError("TTA: need at least one view (views >= 1, or views == 0 with clean=True)")
        if not (float(self.sigma) >= 0.0) or float(self.sigma) == float("inf"):
            raise ValueError("TTA: sigma must be finite and >= 0")
        if not 0 <= int(self.seed) < 2 ** 64:
            raise ValueError("TTA: seed must fit 64 bits")
        return ([None] if self.clean else []) + list(range(v))


def _check_blocks(tta: TTA, members: int):
    blocks = tta.pairs()
    if members * len(blocks) > MAX_BLOCKS:
        raise ValueError(f"TTA: {members} members x {len(blocks)} blocks, cmlpl_ensemble_views takes up to {MAX_BLOCKS}")
    return blocks


def _block(t, g=None):
    """(t, g) of a block given as a view index (None: the clean window), as a (t, g) pair of ``TTA.pairs()``, or with ``g``"""
    if isinstance(t, tuple):
        if g is not None:
            raise ValueError("TTA: a (t, g) block and g")
        t, g = t
    g = 0 if g is None else int(g)
    if not 0 <= g <= 7 or (t is None and g != 0):
        raise ValueError("TTA: a spatial element is 0 .. 7, and 0 for the clean block")
    return t, g


def _key(tta: TTA, t, g=None):
    """(sigma, seed, view, element) of a block (``_block``); the clean block is sigma 0 with element 0 (the clean
    forward's launches and bytes)"""
    t, g = _block(t, g)
    return (C.c_float(0.0 if t is None else float(tta.sigma)), C.c_uint64(int(tta.seed)), C.c_uint32(0 if t is None else int(t)),
            C.c_uint32(g))


def _keys(tta: TTA, members: int):
    """the view keys of ``tta``'s blocks for so many members"""
    return [_key(tta, t) for t in _check_blocks(tta, members)]


@torch.no_grad()
def tta_cube(nets, cube: torch.Tensor, spectra: torch.Tensor, tta: TTA, pixel0: int = 0, n: Optional[int] = None,
             chunk: int = 65536, weights: Optional[Sequence[float]] = None, probs: bool = False, conf: bool = False,
             entropy: bool = False, disagree: bool = False) -> EnsembleResult:
    """``ensemble_cube`` over the views of ``tta``: pixels pixel0 .. pixel0 + n - 1 of the scene (default: all of it),
    ``nets`` as ``cmlpl_amd.ensemble._groups`` takes them (1..4 members).  Every window shape ``infer_supported`` accepts.
    Asynchronous."""
    return _ensemble(nets, cube, spectra, _Range(pixel0, n), lambda M: _keys(tta, M), chunk, weights,
                     (probs, conf, entropy, disagree))


@torch.no_grad()
def tta_pixels(nets, cube: torch.Tensor, spectra: torch.Tensor, pix: torch.Tensor, tta: TTA,
               spec_rows: Optional[torch.Tensor] = None, chunk: int = 65536, weights: Optional[Sequence[float]] = None,
               probs: bool = False, conf: bool = False, entropy: bool = False, disagree: bool = False,
               check: bool = True) -> EnsembleResult:
    """``tta_cube`` for a LIST of scene pixels, through the list-fed forward (``ensemble_pixels``' addressing: item i's
    spectrum is row ``spec_rows[i]`` of ``spectra``, or row i; its VIEW is that of scene pixel ``pix[i]`` either way).
    ``(engine, None)`` scores both networks in one forward launch chain per view.  ``check``: one synchronising range
    check of the lists.  Asynchronous otherwise."""
    return _ensemble(nets, cube, spectra, _List(pix, spec_rows, check), lambda M: _keys(tta, M), chunk, weights,
                     (probs, conf, entropy, disagree))


@torch.no_grad()
def views_of(cube: torch.Tensor, spectra: Optional[torch.Tensor], pix: torch.Tensor, window: int, tta: TTA, t,
             spec_rows: Optional[torch.Tensor] = None, g: Optional[int] = None):
    """view ``t`` of the scene pixels ``pix`` (int64 cuda [n]) as tensors: the windows [n, C, window, window] and -- when
    ``spectra`` is given -- the spectra [n, bands] (row ``spec_rows[i]``, or row ``pix[i]`` of the whole scene's spectra
    when ``spec_rows`` is None) with the view's noise: what the fused forward forms in registers (``cmlpl_tta_patches``).
    ``t=None``: the clean windows and rows.  ``g`` (or ``t`` as a (t, g) pair): the windows under that spatial element.
    Asynchronous."""
    _check_scene(cube, spectra)
    if not (pix.is_cuda and pix.dtype == torch.int64 and pix.dim() == 1 and pix.is_contiguous() and pix.numel() >= 1):
        raise ValueError("pix: need a non-empty contiguous int64 cuda vector")
    tta.blocks()
    sigma, seed, view, sym = _key(tta, t, g)
    rows, cols, Cc = cube.shape
    n, dev = pix.numel(), cube.device
    xp = torch.empty(n, Cc, window, window, dtype=torch.float32, device=dev)
    sr = pix if spec_rows is None else spec_rows
    x = None if spectra is None else torch.empty(n, spectra.shape[1], dtype=torch.float32, device=dev)
    st = _lib.stream(dev)
    _lib.check("cmlpl_tta_patches_sym", _lib.load().cmlpl_tta_patches_sym(
        cube.data_ptr(), rows, cols, Cc, int(window), pix.data_ptr(), n, xp.data_ptr(),
        _lib.ptr(spectra), None if spectra is None else sr.data_ptr(),
        0 if spectra is None else spectra.shape[1], _lib.ptr(x), sigma, seed, view, st, sym))
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
    st = _lib.stream(logits.device)
    _reduce(_lib.load(), logits.data_ptr(), M, V, logits.stride(0), logits.stride(1), _weights(weights, M), n, K, res, 0, st)
    return res


@torch.no_grad()
def infer_cube_view(net, cube: torch.Tensor, spectra: torch.Tensor, tta: TTA, t, pixel0: int = 0,
                    n: Optional[int] = None, chunk: int = 65536, g: Optional[int] = None):
    """``infer_cube(want_logits=True)`` of ONE network on view ``t`` (None: the clean window; a (t, g) pair or ``g``: under
    that spatial element) of pixels pixel0 .. pixel0 + n - 1: (labels int64 [n], logits [n, K]) -- one block of what
    ``tta_cube`` reduces.  Asynchronous."""
    tta.blocks()
    return _infer(net, cube, spectra, _Range(pixel0, n), chunk, True, _key(tta, t, g))


@torch.no_grad()
def infer_pixels_view(nets, cube: torch.Tensor, spectra: torch.Tensor, pix: torch.Tensor, tta: TTA, t,
                      spec_rows: Optional[torch.Tensor] = None, chunk: int = 65536, check: bool = True,
                      g: Optional[int] = None):
    """``infer_pixels(want_logits=True)`` on view ``t`` (None: clean; a (t, g) pair or ``g``: under that spatial element) of
    a pixel list, ``nets`` as ``infer_pixels`` takes them: (labels [n] or [2, n], logits [n, K] or [2, n, K]).
    Asynchronous but for ``check``."""
    tta.blocks()
    return _infer(nets, cube, spectra, _List(pix, spec_rows, check), chunk, True, _key(tta, t, g))
