"""Validation on a split's labelled pixels, on the device (the reference's per-epoch helper ``test_acc``,
tools/hyper_tools.py:372-413, streams a DataLoader of materialised patches and counts on the host).

A split is registered ONCE -- the resident scene cube, the split's spectra, labels and one scene pixel per row
(``HSIDataSet(dataID, 'test').scene_arrays(device)``) -- and an evaluation is then launches only: the list-fed fused eval
forward labels the list under both networks in one call (cmlpl_infer_pixels), the confusion matrices are counted where the
labels lie (cmlpl_confusion), and what leaves the device is nets x K x K integers, not a label image.  ``metrics`` turns a
matrix into OA / Kappa / per-class accuracy / AA with ``tools.hyper_tools.CalAccuracy``'s conventions, in fp64 on the
host."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from .infer import _infer_pixels_into, _nets_buffers, check_pixel_list


class Evaluator:
    """``Evaluator(shape, cube, spectra, truth, pix, spec_rows=None)``: item i of the split is the window of scene pixel
    ``pix[i]`` of ``cube`` [rows, cols, C], the spectrum ``spectra[i]`` (``spectra[spec_rows[i]]`` when ``spec_rows`` is
    given) and the label ``truth[i]`` (int64; outside 0 .. K - 1 = unlabelled: counted in ``ignored``, in no matrix).
    The lists' ranges are checked here, once (one synchronisation); ``evaluate`` neither synchronises nor -- for lists of up
    to ``chunk`` items and windows the fused forward takes -- allocates."""

    def __init__(self, shape, cube: torch.Tensor, spectra: torch.Tensor, truth: torch.Tensor, pix: torch.Tensor,
                 spec_rows: Optional[torch.Tensor] = None, chunk: int = 65536):
        self.lib = _lib.load()
        self.shape = shape
        self.cshape = _lib.Shape(shape.C, shape.H, shape.W, shape.bands, shape.K)
        if not (cube.is_cuda and cube.dtype == torch.float32 and cube.is_contiguous() and cube.dim() == 3
                and cube.shape[2] == shape.C):
            raise ValueError("cube: need contiguous float32 cuda tensor [rows, cols, C]")
        if not (spectra.is_cuda and spectra.dtype == torch.float32 and spectra.is_contiguous() and spectra.dim() == 2
                and spectra.shape[1] == shape.bands):
            raise ValueError("spectra: need contiguous float32 cuda tensor [., bands]")
        rows, cols, _ = cube.shape
        check_pixel_list(pix, rows * cols)
        n = pix.numel()
        if spec_rows is not None:
            check_pixel_list(spec_rows, spectra.shape[0], "spec_rows")
        if (spec_rows is not None and spec_rows.numel() != n) or (spec_rows is None and spectra.shape[0] < n):
            raise ValueError("spectra / spec_rows do not cover the pixel list")
        if not (truth.is_cuda and truth.dtype == torch.int64 and truth.is_contiguous() and tuple(truth.shape) == (n,)):
            raise ValueError("truth: need contiguous int64 cuda vector, one label per list entry")
        if rows < shape.H // 2 or cols < shape.W // 2:
            raise ValueError("scene smaller than half a window")
        self.cube, self.spectra, self.truth, self.pix, self.spec_rows, self.n = cube, spectra, truth, pix, spec_rows, n
        dev = cube.device
        K = shape.K
        self.labels = torch.empty(2, n, dtype=torch.int64, device=dev)
        self.cm = torch.zeros(2, K, K, dtype=torch.int64, device=dev)
        self.ignored = torch.zeros(1, dtype=torch.int64, device=dev)
        self.chunk = max(8, min(int(chunk), n))
        need = self.lib.cmlpl_eval_workspace_bytes(C.byref(self.cshape), 2, self.chunk)
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None     # None: windows go by patches
        self.logits = self.ens_labels = self.cm_ens = None       # evaluate(ensemble=True) creates them at its first call

    @torch.no_grad()
    def evaluate(self, nets, ensemble: bool = False) -> torch.Tensor:
        """confusion matrices int64 [nets, K, K] on the device (row = true class, column = predicted class) of the
        registered split under ``nets`` -- what ``cmlpl_amd.infer.infer_pixels`` takes: ``(TrainEngine, None)`` for both
        networks of an engine, one network, or a pair of modules.  A view of this object's buffer: the next call
        overwrites it.  On the current stream, no synchronisation.
        ``ensemble``: [nets + 1, K, K] -- the same matrices, then the one of the networks' equally weighted ensemble
        (``cmlpl_ensemble`` over the logits of the same forward: the label of the averaged softmax, first maximum).  Its
        buffers (the logits, the ensemble's labels, the matrices) are created at the first such call."""
        cs, nn, flat, pstride, packed, kstride, _ = _nets_buffers(nets)
        if (cs.C, cs.H, cs.W, cs.bands, cs.K) != tuple(getattr(self.cshape, k) for k in ("C", "H", "W", "bands", "K")):
            raise ValueError("the networks' shape is not the registered split's")
        labels = self.labels[:nn]
        logits = None
        if ensemble:
            if self.cm_ens is None:
                dev = self.cube.device
                self.logits = torch.empty(2, self.n, cs.K, dtype=torch.float32, device=dev)
                self.ens_labels = torch.empty(self.n, dtype=torch.int64, device=dev)
                self.cm_ens = torch.zeros(3, cs.K, cs.K, dtype=torch.int64, device=dev)
            logits = self.logits.view(-1)[:nn * self.n * cs.K].view(nn, self.n, cs.K)
        _infer_pixels_into(self.lib, cs, nn, flat, pstride, packed, kstride, self.cube, self.spectra, self.spec_rows,
                           self.pix, labels, logits, self.ws, self.chunk)
        cm = self.cm_ens[:nn + 1] if ensemble else self.cm[:nn]
        cm.zero_()
        self.ignored.zero_()
        st = C.c_void_p(torch.cuda.current_stream(self.cube.device).cuda_stream)
        _lib.check("cmlpl_confusion", self.lib.cmlpl_confusion(
            labels.data_ptr(), nn, self.truth.data_ptr(), self.n, cs.K, cm.data_ptr(), self.ignored.data_ptr(), st))
        if ensemble:
            _lib.check("cmlpl_ensemble", self.lib.cmlpl_ensemble(
                logits.data_ptr(), nn, self.n * cs.K, None, self.n, cs.K, self.ens_labels.data_ptr(), None, None, None,
                None, st))
            _lib.check("cmlpl_confusion", self.lib.cmlpl_confusion(
                self.ens_labels.data_ptr(), 1, self.truth.data_ptr(), self.n, cs.K, cm[nn].data_ptr(), None, st))
        return cm

    @staticmethod
    def metrics(cm):
        """(OA, Kappa, producerA, AA) of ONE confusion matrix [K, K] (device or host integers), fp64 on the host, with
        ``CalAccuracy``'s conventions: the class count is the largest class that OCCURS in the truth plus one (rows past it
        are empty and dropped; predictions past it are counted in the last kept column, as its clip does), a class
        without a sample has producer's accuracy 0, AA is the mean over the kept classes."""
        return metrics(cm)


def metrics(cm):
    m = cm.detach().cpu().numpy() if isinstance(cm, torch.Tensor) else np.asarray(cm)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("metrics: one square matrix")
    present = np.nonzero(m.sum(1))[0]
    if present.size == 0:
        raise ValueError("metrics: the matrix is empty")
    n = int(present.max()) + 1
    c = np.zeros((n, n), dtype=np.float64)
    c[:, :] = m[:n, :n]
    c[:, n - 1] += m[:n, n:].sum(1)
    total = c.sum()
    OA = np.trace(c) / total
    pe = float((c.sum(0) * c.sum(1)).sum()) / (total * total)
    Kappa = (OA - pe) / (1.0 - pe) if pe < 1.0 else 0.0
    producerA = np.diag(c) / np.maximum(c.sum(1), 1.0)
    return OA, Kappa, producerA, float(np.mean(producerA))
