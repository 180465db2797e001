"""Ensemble prediction of the trained networks: averaged class probabilities, the label they give, its confidence, the
entropy and the members' disagreement, on the device (``cmlpl_ensemble``, csrc/ensemble.hip; the reference reports each
network alone and only ever a hard label).

Per pixel: ``p_m = softmax(z_m)`` of every member in fp32, ``p = sum_m w_m p_m`` (m ascending, the weights normalised on
the host), ``label`` = the first maximum of ``p`` (a NaN counts as the maximum, the first NaN wins: ``torch.max``'s rule),
``conf = p[label]``, ``entropy = -sum_c p_c log p_c`` (0 log 0 = 0) and ``disagree`` = how many members' own first-maximum
label differs from ``label``.  Members are 1..4 networks -- Base and Base1, their EMA teachers, or loaded modules.

``ensemble_logits`` is the launch on logits that exist; ``ensemble_cube`` / ``ensemble_pixels`` are ``_ensemble`` -- the
chunk loop of ``cmlpl_amd.infer`` with a reduction behind each chunk -- on the one clean block, as ``cmlpl_amd.tta`` is on
the blocks of a ``TTA``.  Nothing here synchronises; everything runs on the current stream."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from .infer import _check_feed, _check_scene, _Forward, _List, _nets_buffers, _predict, _Range, _same_shape

MAX_MEMBERS = 4


class EnsembleResult(NamedTuple):
    labels: torch.Tensor                        # int64 [n]
    probs: Optional[torch.Tensor] = None        # float32 [n, K]
    conf: Optional[torch.Tensor] = None         # float32 [n]
    entropy: Optional[torch.Tensor] = None      # float32 [n]
    disagree: Optional[torch.Tensor] = None     # int32 [n]


def _weights(weights, members: int):
    """the host array cmlpl_ensemble reads (None: equal weights); the library checks the values"""
    if weights is None:
        return None
    w = [float(v) for v in weights]
    if len(w) != members:
        raise ValueError(f"weights: {len(w)} values for {members} members")
    return (C.c_float * members)(*w)


def _alloc(n: int, K: int, dev, probs: bool, conf: bool, entropy: bool, disagree: bool) -> EnsembleResult:
    return EnsembleResult(
        torch.empty(n, dtype=torch.int64, device=dev),
        torch.empty(n, K, dtype=torch.float32, device=dev) if probs else None,
        torch.empty(n, dtype=torch.float32, device=dev) if conf else None,
        torch.empty(n, dtype=torch.float32, device=dev) if entropy else None,
        torch.empty(n, dtype=torch.int32, device=dev) if disagree else None)


def _reduce(lib, z_ptr: int, M: int, V, ms: int, vs: int, cw, n: int, K: int, res: EnsembleResult, o: int, stream):
    """one cmlpl_ensemble (``V`` None) or cmlpl_ensemble_views (V views) over n pixels of M members, the blocks ``ms`` /
    ``vs`` floats apart; the results go to rows o .. o + n - 1 of ``res``"""
    at = lambda t, size: None if t is None else t.data_ptr() + size * o
    outs = (at(res.labels, 8), at(res.probs, 4 * K), at(res.conf, 4), at(res.entropy, 4), at(res.disagree, 4), stream)
    if V is None:
        _lib.check("cmlpl_ensemble", lib.cmlpl_ensemble(z_ptr, M, ms, cw, n, K, *outs))
    else:
        _lib.check("cmlpl_ensemble_views", lib.cmlpl_ensemble_views(z_ptr, M, V, ms, vs, cw, n, K, *outs))


@torch.no_grad()
def ensemble_logits(logits: torch.Tensor, weights: Optional[Sequence[float]] = None, probs: bool = False,
                    conf: bool = False, entropy: bool = False, disagree: bool = False) -> EnsembleResult:
    """The ensemble of logits [M, n, K] (float32 cuda, contiguous in its last two dimensions; [n, K] is one member):
    ``labels`` and whatever was asked for.  One launch on the current stream, no synchronisation."""
    if logits.dim() == 2:
        logits = logits.unsqueeze(0)
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3):
        raise ValueError("logits: need a float32 cuda tensor [M, n, K]")
    M, n, K = logits.shape
    if logits.stride(2) != 1 or logits.stride(1) != K or (M > 1 and logits.stride(0) < n * K):
        raise ValueError("logits: the last two dimensions must be contiguous, the members one after another")
    if not 1 <= M <= MAX_MEMBERS:
        raise ValueError(f"logits: {M} members, the ensemble takes 1 .. {MAX_MEMBERS}")
    res = _alloc(n, K, logits.device, probs, conf, entropy, disagree)
    st = _lib.stream(logits.device)
    _reduce(_lib.load(), logits.data_ptr(), M, None, logits.stride(0) if M > 1 else n * K, 0, _weights(weights, M), n, K, res, 0, st)
    return res


def _is_net_pair(x) -> bool:
    """``(engine, None)`` / ``(engine.teacher, None)``: both networks of an engine, or of its teacher"""
    return isinstance(x, tuple) and len(x) == 2 and x[1] is None and hasattr(x[0], "params")


def _groups(nets):
    """``nets`` as a list of what ``infer_pixels`` takes, each with its number of members: the entries of a list (or of a
    tuple of modules) are one network each (a BaseNet2 module, ``(engine, i)``, ``(engine.teacher, i)``) or a pair
    ``(engine, None)``; anything else is ONE such entry."""
    if isinstance(nets, list):
        entries = nets
    elif isinstance(nets, tuple) and len(nets) >= 1 and not hasattr(nets[0], "params"):
        entries = list(nets)
    else:
        entries = [nets]
    groups = [(e, 2 if _is_net_pair(e) else 1) for e in entries]
    members = sum(k for _, k in groups)
    if not 1 <= members <= MAX_MEMBERS:
        raise ValueError(f"nets: {members} members, the ensemble takes 1 .. {MAX_MEMBERS}")
    return groups, members


def _ensemble(nets, cube, spectra, feed, keys, chunk, weights, asks) -> EnsembleResult:
    """``ensemble_*`` (``keys`` None: the one clean block, reduced by cmlpl_ensemble) and ``cmlpl_amd.tta.tta_*`` (``keys``:
    the view keys of a ``TTA`` for a number of members, reduced by cmlpl_ensemble_views) on a feed of ``cmlpl_amd.infer``:
    per chunk every block x member forward writes into one reused buffer [blocks, members, chunk, K] and one reduction
    follows.  The range feed runs one network per forward, the list feed a pair ``(engine, None)`` in one launch chain."""
    groups, M = _groups(nets)
    keys = None if keys is None else keys(M)
    if isinstance(feed, _Range):
        groups = [(m, 1) for e, k in groups for m in ([(e[0], 0), (e[0], 1)] if k == 2 else [e])]
    bufs = [_nets_buffers(e) for e, _ in groups]
    cs = _same_shape(bufs)
    _check_scene(cube, spectra, cs, whole=isinstance(feed, _Range))
    n = _check_feed(cube, spectra, feed)
    cw = _weights(weights, M)
    lib, dev, K = _lib.load(), cube.device, cs.K
    V = None if keys is None else len(keys)
    fwd = _Forward(lib, cs, max(b[1] for b in bufs), cube, spectra, feed, n, chunk, views=keys is not None, labels=False)
    res = _alloc(n, K, dev, *asks)
    buf = torch.empty((V or 1) * M * fwd.chunk * K, dtype=torch.float32, device=dev)
    st = _lib.stream(dev)
    _predict(fwd, bufs, keys or [None], n, buf=buf,
             reduce=lambda z, o, m: _reduce(lib, z.data_ptr(), M, V, m * K, M * m * K, cw, m, K, res, o, st))
    return res


@torch.no_grad()
def ensemble_cube(nets, cube: torch.Tensor, spectra: torch.Tensor, pixel0: int = 0, n: Optional[int] = None,
                  chunk: int = 65536, weights: Optional[Sequence[float]] = None, probs: bool = False, conf: bool = False,
                  entropy: bool = False, disagree: bool = False) -> EnsembleResult:
    """The ensemble of ``nets`` (see ``_groups``) on pixels pixel0 .. pixel0 + n - 1 of the scene (default: all of it).
    Every window shape ``infer_supported`` accepts, the by-patches path included.  Asynchronous."""
    return _ensemble(nets, cube, spectra, _Range(pixel0, n), None, chunk, weights, (probs, conf, entropy, disagree))


@torch.no_grad()
def ensemble_pixels(nets, cube: torch.Tensor, spectra: torch.Tensor, pix: torch.Tensor,
                    spec_rows: Optional[torch.Tensor] = None, chunk: int = 65536,
                    weights: Optional[Sequence[float]] = None, probs: bool = False, conf: bool = False,
                    entropy: bool = False, disagree: bool = False, check: bool = True) -> EnsembleResult:
    """``ensemble_cube`` for a LIST of scene pixels, through the list-fed forward of ``infer_pixels`` (same addressing:
    item i's spectrum is row ``spec_rows[i]`` of ``spectra``, or row i).  ``(engine, None)`` yields both networks in one
    forward launch chain; a list may hold several such entries (``[(eng, None), (eng.teacher, None)]``: four members).
    ``check``: one synchronising range check of the lists, as in ``infer_pixels``.  Asynchronous otherwise."""
    return _ensemble(nets, cube, spectra, _List(pix, spec_rows, check), None, chunk, weights,
                     (probs, conf, entropy, disagree))
