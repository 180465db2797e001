"""Edge-preserving spatial smoothing of class probability maps, on the device (``cmlpl_smooth_probs``, csrc/smooth.hip;
the reference has no counterpart: each of its labels is the product of a single window).

Every class's probability map is averaged over a (2R + 1) x (2R + 1) neighbourhood; a neighbour counts less the farther
away it is (``sigma_s``, in pixels) and the less its guide vector -- the first ``guide`` channels of the scene cube, its
leading z-scored principal components -- resembles the centre pixel's (``sigma_r``); taps outside the scene are left out.
The new label is the first maximum of the smoothed probabilities, confidence and entropy as in ``cmlpl_amd.ensemble``.
The definition, down to the order of the fp32 operations, is in ``include/cmlpl.h`` ("THE DEFINITION OF A SMOOTHED MAP").

``smooth_probs`` is the launch on probabilities that exist; ``smooth_cube`` is ``ensemble_cube`` (or ``tta_cube``) over
the whole scene followed by it.  Nothing here synchronises; everything runs on the current stream."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from .ensemble import EnsembleResult, _alloc, ensemble_cube

MAX_RADIUS = 8
MAX_GUIDE = 8


class Smooth(NamedTuple):
    """``iters`` passes of the filter with ``radius`` R (a (2R + 1)^2 neighbourhood), spatial width ``sigma_s`` in pixels
    (None: R / 2), guide width ``sigma_r`` in units of the z-scored guide channels (``float('inf')``: the distance in the
    guide does not count) and the first ``guide`` channels of the cube as the guide (0: none; clamped to the cube's
    channels).  The defaults are a starting point, NOT tuned on any scene."""
    radius: int
    sigma_s: Optional[float] = None
    sigma_r: float = 0.5
    guide: int = 3
    iters: int = 1

    def params(self, channels: Optional[int] = None):
        """(radius, sigma_s, sigma_r, guide channels, iters) as the launch takes them, checked; ``channels``: the cube's"""
        R, G, n = int(self.radius), int(self.guide), int(self.iters)
        if not 1 <= R <= MAX_RADIUS:
            raise ValueError(f"Smooth: radius must be 1 .. {MAX_RADIUS}")
        ss = R / 2.0 if self.sigma_s is None else float(self.sigma_s)
        if not (ss > 0.0) or ss == float("inf"):
            raise ValueError("Smooth: sigma_s must be finite and > 0")
        sr = float(self.sigma_r)
        if not (sr > 0.0):
            raise ValueError("Smooth: sigma_r must be > 0 (float('inf'): no guide distance)")
        if not 0 <= G <= MAX_GUIDE:
            raise ValueError(f"Smooth: guide must be 0 .. {MAX_GUIDE} channels")
        if n < 1:
            raise ValueError("Smooth: iters must be >= 1")
        if min(2.0 * ss * ss, 2.0 * sr * sr) < 1.0 / 3.0e38:      # cmlpl_smooth_probs: 1 / (2 sigma^2) must be finite in fp32
            raise ValueError("Smooth: sigma too small")
        return R, ss, sr, (G if channels is None else min(G, int(channels))), n


@torch.no_grad()
def smooth_probs(probs: torch.Tensor, cube: torch.Tensor, smooth: Smooth, probs_out: bool = True, conf: bool = False,
                 entropy: bool = False) -> EnsembleResult:
    """``probs`` [rows * cols, K] (float32 cuda, contiguous: the ``probs`` of an ``EnsembleResult`` over the whole scene)
    smoothed under the guide of ``cube`` [rows, cols, C]: ``labels`` and whatever was asked for (``disagree`` is None).
    ``probs`` is left as it is.  ``iters`` > 1 ping-pongs two buffers and asks only the last pass for labels, confidence
    and entropy.  On the current stream, no synchronisation."""
    if not (cube.is_cuda and cube.dtype == torch.float32 and cube.dim() == 3 and cube.is_contiguous()):
        raise ValueError("cube: need a contiguous float32 cuda tensor [rows, cols, C]")
    rows, cols, Cc = cube.shape
    if not (probs.is_cuda and probs.dtype == torch.float32 and probs.dim() == 2 and probs.is_contiguous()
            and probs.device == cube.device):
        raise ValueError("probs: need a contiguous float32 cuda tensor [rows * cols, K] on the cube's device")
    n, K = probs.shape
    if n != rows * cols:
        raise ValueError(f"probs: {n} rows for a scene of {rows} x {cols} pixels (the filter needs the whole map)")
    R, ss, sr, G, iters = smooth.params(Cc)
    lib, dev = _lib.load(), cube.device
    st = _lib.stream(dev)
    res = _alloc(n, K, dev, probs_out, conf, entropy, False)
    src, bufs = probs, []                # the input is never written: two buffers of our own from the third pass on
    for it in range(iters):
        last = it == iters - 1
        if not last and len(bufs) < 2:
            bufs.append(torch.empty(n, K, dtype=torch.float32, device=dev))
        dst = res.probs if last else bufs[it % 2]
        _lib.check("cmlpl_smooth_probs", lib.cmlpl_smooth_probs(
            src.data_ptr(), cube.data_ptr() if G > 0 else None, cube.stride(1), G, rows, cols, K, R, ss, sr, _lib.ptr(dst),
            res.labels.data_ptr() if last else None, _lib.ptr(res.conf) if last else None,
            _lib.ptr(res.entropy) if last else None, st))
        src = dst
    return res


@torch.no_grad()
def smooth_cube(nets, cube: torch.Tensor, spectra: torch.Tensor, smooth: Smooth, tta=None,
                weights: Optional[Sequence[float]] = None, chunk: int = 65536, probs: bool = False, conf: bool = False,
                entropy: bool = False) -> EnsembleResult:
    """``ensemble_cube(nets, ..., probs=True)`` over the WHOLE scene -- ``tta_cube`` when ``tta`` (a ``cmlpl_amd.tta.TTA``)
    is given -- followed by ``smooth_probs``: the smoothed prediction of ``nets`` (1..4 members, as
    ``cmlpl_amd.ensemble._groups`` takes them).  A pixel range or list has no map to smooth.  Asynchronous."""
    smooth.params(cube.shape[2] if cube.dim() == 3 else None)
    if tta is None:
        raw = ensemble_cube(nets, cube, spectra, chunk=chunk, weights=weights, probs=True)
    else:
        from .tta import tta_cube
        raw = tta_cube(nets, cube, spectra, tta, chunk=chunk, weights=weights, probs=True)
    return smooth_probs(raw.probs, cube, smooth, probs_out=probs, conf=conf, entropy=entropy)
