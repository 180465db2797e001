"""Validation on a split's labelled pixels, on the device (the reference's per-epoch helper ``test_acc``,
tools/hyper_tools.py:372-413, streams a DataLoader of materialised patches and counts on the host).

A split is registered ONCE -- the resident scene cube, the split's spectra, labels and one scene pixel per row
(``HSIDataSet(dataID, 'test').scene_arrays(device)``) -- and an evaluation is then launches only: the list-fed fused eval
forward labels the list under both networks in one call (cmlpl_infer_pixels), the confusion matrices are counted where the
labels lie (cmlpl_confusion), and what leaves the device is nets x K x K integers, not a label image.  ``metrics`` turns a
matrix into OA / Kappa / per-class accuracy / AA with ``tools.hyper_tools.CalAccuracy``'s conventions, in fp64 on the
host."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .infer import _check_feed, _check_scene, _Forward, _List, _nets_buffers, _predict


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
        _check_scene(cube, spectra, self.cshape)
        rows, cols, _ = cube.shape
        feed = _List(pix, spec_rows, True)
        n = _check_feed(cube, spectra, feed)
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
        self.fwd = _Forward(self.lib, self.cshape, 2, cube, spectra, feed, n, chunk)
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
        group = _nets_buffers(nets)
        cs, nn = group[0], group[1]
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
        _predict(self.fwd, [group], [None], self.n, labels, logits)
        cm = self.cm_ens[:nn + 1] if ensemble else self.cm[:nn]
        cm.zero_()
        self.ignored.zero_()
        st = _lib.stream(self.cube.device)
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
