"""Ensemble prediction of the trained networks: averaged class probabilities, the label they give, its confidence, the
entropy and the members' disagreement, on the device (``cmlpl_ensemble``, csrc/ensemble.hip; the reference reports each
network alone and only ever a hard label).

Per pixel: ``p_m = softmax(z_m)`` of every member in fp32, ``p = sum_m w_m p_m`` (m ascending, the weights normalised on
the host), ``label`` = the first maximum of ``p`` (a NaN counts as the maximum, the first NaN wins: ``torch.max``'s rule),
``conf = p[label]``, ``entropy = -sum_c p_c log p_c`` (0 log 0 = 0) and ``disagree`` = how many members' own first-maximum
label differs from ``label``.  Members are 1..4 networks -- Base and Base1, their EMA teachers, or loaded modules.

``ensemble_logits`` is the launch on logits that exist; ``ensemble_cube`` / ``ensemble_pixels`` run the eval forwards of
``cmlpl_amd.infer`` chunk by chunk into one reused logits buffer with one launch behind each chunk.  Nothing here
synchronises; everything runs on the current stream."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from .infer import _infer_pixels_into, _nets_buffers, check_pixel_list, infer_cube

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


def _launch(lib, logits_ptr: int, members: int, stride: int, cw, n: int, K: int, res: EnsembleResult, o: int, stream):
    """one cmlpl_ensemble over n pixels whose results go to rows o .. o + n - 1 of ``res``"""
    at = lambda t, size: None if t is None else t.data_ptr() + size * o
    _lib.check("cmlpl_ensemble", lib.cmlpl_ensemble(
        logits_ptr, members, stride, cw, n, K, at(res.labels, 8), at(res.probs, 4 * K), at(res.conf, 4),
        at(res.entropy, 4), at(res.disagree, 4), stream))


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
    st = C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)
    _launch(_lib.load(), logits.data_ptr(), M, logits.stride(0) if M > 1 else n * K, _weights(weights, M), n, K, res, 0, st)
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


@torch.no_grad()
def ensemble_cube(nets, cube: torch.Tensor, spectra: torch.Tensor, pixel0: int = 0, n: Optional[int] = None,
                  chunk: int = 65536, weights: Optional[Sequence[float]] = None, probs: bool = False, conf: bool = False,
                  entropy: bool = False, disagree: bool = False) -> EnsembleResult:
    """The ensemble of ``nets`` (see ``_groups``) on pixels pixel0 .. pixel0 + n - 1 of the scene (default: all of it):
    per chunk every member's ``infer_cube(want_logits=True)`` writes its logits into one reused buffer of
    members x chunk x K floats, and one ``cmlpl_ensemble`` follows.  Every window shape ``infer_supported`` accepts, the
    by-patches path included.  Asynchronous."""
    groups, M = _groups(nets)
    members = []
    for e, k in groups:
        members += [(e[0], 0), (e[0], 1)] if k == 2 else [e]
    if not (cube.is_cuda and cube.dim() == 3):
        raise ValueError("cube: need contiguous float32 cuda tensor [rows, cols, C]")
    rows, cols, _ = cube.shape
    n = rows * cols - pixel0 if n is None else int(n)
    if pixel0 < 0 or n < 1 or pixel0 + n > rows * cols:
        raise ValueError("pixel range outside the scene")
    K = _nets_buffers(members[0])[0].K
    cw = _weights(weights, M)
    lib, dev = _lib.load(), cube.device
    chunk = max(8, min(int(chunk), n))
    res = _alloc(n, K, dev, probs, conf, entropy, disagree)
    buf = torch.empty(M * chunk * K, dtype=torch.float32, device=dev)
    own = torch.empty(chunk, dtype=torch.int64, device=dev)            # a member's own argmax: written, not used
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        z = buf[:M * m * K].view(M, m, K)
        for k, net in enumerate(members):
            infer_cube(net, cube, spectra, pixel0 + o, m, chunk=chunk, want_logits=True, out=(own[:m], z[k]))
        _launch(lib, z.data_ptr(), M, m * K, cw, m, K, res, o, st)
    return res


@torch.no_grad()
def ensemble_pixels(nets, cube: torch.Tensor, spectra: torch.Tensor, pix: torch.Tensor,
                    spec_rows: Optional[torch.Tensor] = None, chunk: int = 65536,
                    weights: Optional[Sequence[float]] = None, probs: bool = False, conf: bool = False,
                    entropy: bool = False, disagree: bool = False, check: bool = True) -> EnsembleResult:
    """``ensemble_cube`` for a LIST of scene pixels, through the list-fed forward of ``infer_pixels`` (same addressing:
    item i's spectrum is row ``spec_rows[i]`` of ``spectra``, or row i).  ``(engine, None)`` yields both networks in one
    forward launch chain; a list may hold several such entries (``[(eng, None), (eng.teacher, None)]``: four members).
    ``check``: one synchronising range check of the lists, as in ``infer_pixels``.  Asynchronous otherwise."""
    groups, M = _groups(nets)
    if not (cube.is_cuda and cube.dtype == torch.float32 and cube.is_contiguous() and cube.dim() == 3):
        raise ValueError("cube: need contiguous float32 cuda tensor [rows, cols, C]")
    rows, cols, Cc = cube.shape
    if not (spectra.is_cuda and spectra.dtype == torch.float32 and spectra.is_contiguous() and spectra.dim() == 2):
        raise ValueError("spectra: need contiguous float32 cuda tensor [., bands]")
    bufs = [_nets_buffers(e) for e, _ in groups]
    cs = bufs[0][0]
    for b in bufs:
        if (b[0].C, b[0].H, b[0].W, b[0].bands, b[0].K) != (cs.C, cs.H, cs.W, cs.bands, cs.K):
            raise ValueError("the networks differ in shape")
    if Cc != cs.C or spectra.shape[1] != cs.bands:
        raise ValueError(f"cube has {Cc} channels / spectra {spectra.shape[1]} bands, the network wants {cs.C} / {cs.bands}")
    if check:
        check_pixel_list(pix, rows * cols)
        if spec_rows is not None:
            check_pixel_list(spec_rows, spectra.shape[0], "spec_rows")
    n = pix.numel()
    if (spec_rows is not None and spec_rows.numel() != n) or (spec_rows is None and spectra.shape[0] < n):
        raise ValueError("spectra / spec_rows do not cover the pixel list")
    K = cs.K
    cw = _weights(weights, M)
    lib, dev = _lib.load(), cube.device
    chunk = max(8, min(int(chunk), n))
    res = _alloc(n, K, dev, probs, conf, entropy, disagree)
    buf = torch.empty(M * chunk * K, dtype=torch.float32, device=dev)
    own = torch.empty(2 * chunk, dtype=torch.int64, device=dev)        # the members' own argmax: written, not used
    wss = []
    for b in bufs:
        need = lib.cmlpl_eval_workspace_bytes(C.byref(b[0]), b[1], chunk)
        wss.append(torch.empty(need, dtype=torch.uint8, device=dev) if need else None)      # None: windows go by patches
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        z = buf[:M * m * K].view(M, m, K)
        k = 0
        for (bcs, nn, flat, pstride, packed, kstride, _), ws in zip(bufs, wss):
            _infer_pixels_into(lib, bcs, nn, flat, pstride, packed, kstride, cube,
                               spectra if spec_rows is not None else spectra[o:o + m],
                               None if spec_rows is None else spec_rows[o:o + m], pix[o:o + m],
                               own[:nn * m].view(nn, m), z[k:k + nn], ws, chunk)
            k += nn
        _launch(lib, z.data_ptr(), M, m * K, cw, m, K, res, o, st)
    return res
