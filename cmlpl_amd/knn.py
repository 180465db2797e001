"""kNN evaluation of the spectral embedding: embed, search, vote (include/cmlpl.h, "THE DEFINITION OF A kNN VOTE").

Two of the method's three loss terms act on ``feat``, the 1024-wide L2-normalised output of the spectral branch
(tools/models.py:142-146); the memory banks hold its rows and the pseudo-label graph is built from its cosine similarities.
``embed`` returns it for listed spectra rows (``cmlpl_embed``: the two launches the eval forward uses, no window, no cube);
``knn`` is the weighted kNN classifier of Wu et al. (CVPR 2018) over such rows -- a query takes the labels of its k most
similar gallery rows, each weighted by ``exp(s / T)`` -- in one streaming pass (``cmlpl_knn``, csrc/knn.hip: the [n][m]
similarity matrix never exists); ``KnnEvaluator`` registers a gallery and a query list once and turns a pair of networks
into confusion matrices with launches only.  Its gap to the linear head says whether the contrastive terms or the
classifier carry a result.  ``knn_host`` / ``vote_host`` restate the definition in numpy: they touch no GPU, and the tests
hold the kernel to them."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

D = 1024
K_MAX, NBR_MAX = 64, 32


def inv_T_of(T: float) -> float:
    """inv_T = fl32(1 / T), formed in double"""
    T = float(T)
    if not (T > 0.0 and np.isfinite(T)):
        raise ValueError("T: a finite temperature > 0")
    v = float(np.float32(1.0 / T))
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError("T: 1 / T is no positive float32")
    return v


def _np(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def purity(nbr_idx, gallery_labels, truth) -> float:
    """the mean, over the queries that have a neighbour, of the share of a query's neighbours that carry its true class"""
    idx, lab, t = _np(nbr_idx).astype(np.int64), _np(gallery_labels).astype(np.int64), _np(truth).astype(np.int64)
    have = idx >= 0
    same = have & (lab[np.where(have, idx, 0)] == t[:, None])
    cnt = have.sum(1)
    rows = cnt > 0
    return float((same.sum(1)[rows] / cnt[rows]).mean()) if rows.any() else float("nan")


class KnnResult(NamedTuple):
    """what ``knn`` returns; a field that was not asked for is None"""
    labels: object          # int64 [n]: the first maximum of probs, -1 for a query without a candidate
    probs: object           # float32 [n, K]: the vote (a NaN row for a query without a candidate)
    nbr_idx: object         # int32 [n, k]: gallery indices by rank, -1 past the last candidate
    nbr_sim: object         # float32 [n, k]: their similarities, -inf past the last candidate

    def purity(self, gallery_labels, truth) -> float:
        if self.nbr_idx is None:
            raise ValueError("purity: a result of knn(..., neighbours=True)")
        return purity(self.nbr_idx, gallery_labels, truth)


# ------------------------------------------------------------------ the definition, restated in numpy
class KnnHost(NamedTuple):
    nbr_idx: np.ndarray     # int32 [n, k]
    nbr_sim: np.ndarray     # float64 [n, k]: the fp64 similarities
    probs: np.ndarray       # float64 [n, K]: the vote in fp64 (None without labels)
    labels: np.ndarray      # int64 [n]: its first maximum
    probs32: np.ndarray     # float32 [n, K]: the header's fp32 chain on fl32 of the fp64 similarities
    labels32: np.ndarray

    def purity(self, gallery_labels, truth) -> float:
        return purity(self.nbr_idx, gallery_labels, truth)


def vote_host(nbr_idx, nbr_sim, gallery_labels, K: int, T: float):
    """The vote over given neighbour lists (rank order, idx -1 / sim -inf past the end): (probs fp64, labels, probs32,
    labels32) -- in fp64, and the header's fp32 chain: w_r = expf(fl32(fl32(s_r - s_0) inv_T)), den and score accumulated r
    ascending, p = score / den, the first maximum.  Both use the same inv_T = fl32(1 / T)."""
    idx = np.asarray(nbr_idx, np.int64)
    n, k = idx.shape
    lab = np.asarray(gallery_labels, np.int64)
    have = idx >= 0
    nl = np.where(have, lab[np.where(have, idx, 0)], -1)
    inv = inv_T_of(T)
    out = []
    for dt in (np.float64, np.float32):
        s = np.asarray(nbr_sim).astype(dt)
        with np.errstate(all="ignore"):
            w = np.exp(((s - s[:, :1]).astype(dt) * dt(inv)).astype(dt)).astype(dt)
        w = np.where(have, w, dt(0))
        den = np.zeros(n, dt)
        score = np.zeros((n, K), dt)
        for r in range(k):                                                  # ascending
            den = (den + w[:, r]).astype(dt)
            rows = np.nonzero(have[:, r])[0]
            score[rows, nl[rows, r]] = (score[rows, nl[rows, r]] + w[rows, r]).astype(dt)
        with np.errstate(all="ignore"):
            p = (score / den[:, None]).astype(dt)
        none = ~have[:, 0]
        p[none] = np.nan
        out += [p, np.where(none, -1, np.where(none[:, None], 0, p).argmax(1)).astype(np.int64)]
    return tuple(out)


def knn_host(query, gallery, gallery_labels, K: int, k: int, T: float = 1.0, skip=None) -> KnnHost:
    """The definition: fp64 similarities, the candidates, the order (s descending, j ascending), the vote."""
    q, g = np.asarray(query, np.float32).astype(np.float64), np.asarray(gallery, np.float32).astype(np.float64)
    n, m = q.shape[0], g.shape[0]
    if not 1 <= k <= NBR_MAX:
        raise ValueError("k: 1 .. 32")
    with np.errstate(all="ignore"):
        S = q @ g.T
    ok = np.isfinite(S)
    if skip is not None:
        sk = np.asarray(skip, np.int64).reshape(-1)
        ok &= np.arange(m)[None, :] != sk[:, None]
    if gallery_labels is not None:
        lab = np.asarray(gallery_labels, np.int64).reshape(-1)
        if not 1 <= K <= K_MAX:
            raise ValueError("K: 1 .. 64")
        ok &= ((lab >= 0) & (lab < K))[None, :]
    key = np.where(ok, -S, np.inf)
    key = np.where(key == 0, 0.0, key)                                       # +0 and -0 are equal: the index decides
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    if order.shape[1] < k:
        order = np.concatenate([order, np.zeros((n, k - order.shape[1]), order.dtype)], 1)
    have = np.arange(k)[None, :] < ok.sum(1)[:, None]
    idx = np.where(have, order, -1).astype(np.int32)
    sim = np.where(have, np.take_along_axis(np.where(ok, S, -np.inf), order, 1), -np.inf)
    if gallery_labels is None:
        return KnnHost(idx, sim, None, None, None, None)
    return KnnHost(idx, sim, *vote_host(idx, sim, lab, K, T))


# ------------------------------------------------------------------ the device side
def _rows_ok(t, name):
    import torch
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == D and t.is_contiguous() and t.shape[0] >= 1):
        raise ValueError(f"{name}: need a contiguous float32 cuda tensor [rows, {D}], at least one row")


def _list_ok(t, n, name, dev):
    import torch
    if not (t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous() and t.shape[0] == n and t.device == dev):
        raise ValueError(f"{name}: need a contiguous int64 cuda vector of {n} entries on the device of the rows")


def embed(nets, spectra, spec_rows=None, out=None):
    """(feat float32 [n, 1024], norm float32 [n]) of the listed spectra rows -- [2, n, 1024] / [2, n] for two networks:
    item i is row ``spec_rows[i]`` of ``spectra`` [., bands] (row i without a list; the list is followed without a bounds
    check).  ``nets`` is what ``cmlpl_amd.infer._nets_buffers`` takes: ``(engine, None)``, ``(engine, i)``, one module, a
    pair of modules, ``(eng.teacher, None)``.  ``norm`` is the row's length before the division: a zero there marks a
    dead-ReLU row, whose ``feat`` row is NaN.  Bit-equal to the ``feat`` of the eval forward.  Two launches on the current
    stream, no synchronisation.  ``out``: (feat, norm) buffers to write instead of new tensors."""
    import torch
    from . import _lib
    from .infer import _nets_buffers
    cs, nn, flat, pstride, _, _, squeeze = _nets_buffers(nets)
    if not (spectra.is_cuda and spectra.dtype == torch.float32 and spectra.dim() == 2 and spectra.is_contiguous()
            and spectra.shape[1] == cs.bands):
        raise ValueError(f"spectra: need a contiguous float32 cuda tensor [., {cs.bands}]")
    dev = spectra.device
    n = spectra.shape[0] if spec_rows is None else spec_rows.shape[0]
    if n < 1:
        raise ValueError("embed: at least one row")
    if spec_rows is not None:
        _list_ok(spec_rows, n, "spec_rows", dev)
    if out is None:
        feat = torch.empty(nn, n, D, dtype=torch.float32, device=dev)
        norm = torch.empty(nn, n, dtype=torch.float32, device=dev)
    else:
        feat, norm = out
        if not (feat.is_cuda and feat.dtype == torch.float32 and feat.is_contiguous() and feat.numel() == nn * n * D
                and norm.is_cuda and norm.dtype == torch.float32 and norm.is_contiguous() and norm.numel() == nn * n):
            raise ValueError("out: contiguous float32 cuda buffers [nets, n, 1024] and [nets, n]")
    _lib.check("cmlpl_embed", _lib.load().cmlpl_embed(
        C.byref(cs), nn, flat.data_ptr(), pstride, spectra.data_ptr(), _lib.ptr(spec_rows),
        n, feat.data_ptr(), norm.data_ptr(), _lib.stream(dev)))
    if out is None and squeeze:
        return feat[0], norm[0]
    return feat, norm


def workspace_bytes(n: int, m: int, k: int) -> int:
    from . import _lib
    need = _lib.load().cmlpl_knn_workspace_bytes(int(n), int(m), int(k))
    if need == 0:
        raise ValueError("knn: n, m >= 1 and 1 <= k <= 32")
    return need


def knn(query, gallery, gallery_labels, K: int, k: int, T: float = 1.0, skip=None, probs: bool = True,
        neighbours: bool = False, workspace=None) -> KnnResult:
    """The kNN vote of every row of ``query`` [n, 1024] over ``gallery`` [m, 1024] (float32 cuda, rows of unit length):
    ``gallery_labels`` int64 cuda [m] (a label outside 0 .. K - 1 is never a neighbour), ``skip`` int64 cuda [n] or None (the
    gallery index query i may not take: leave-one-out passes ``arange(n)``), k 1 .. 32 neighbours at temperature T.  With
    ``gallery_labels`` None (and K = 0) it is the search alone: the neighbours, no vote.  Launches on the current stream,
    no synchronisation; ``workspace``: a uint8 cuda buffer of ``workspace_bytes(n, m, k)`` to use instead of a new one."""
    import torch
    from . import _lib
    _rows_ok(query, "query")
    _rows_ok(gallery, "gallery")
    dev = query.device
    n, m = query.shape[0], gallery.shape[0]
    if gallery.device != dev:
        raise ValueError("query and gallery lie on different devices")
    if not 1 <= k <= NBR_MAX:
        raise ValueError("k: 1 .. 32")
    vote = gallery_labels is not None
    if vote:
        _list_ok(gallery_labels, m, "gallery_labels", dev)
        if not 1 <= K <= K_MAX:
            raise ValueError("K: 1 .. 64")
    else:
        K, neighbours = 0, True
    if skip is not None:
        _list_ok(skip, n, "skip", dev)
    need = workspace_bytes(n, m, k)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.numel() >= need):
        raise ValueError(f"workspace: a contiguous uint8 cuda buffer of {need} bytes")
    res = KnnResult(torch.empty(n, dtype=torch.int64, device=dev) if vote else None,
                    torch.empty(n, K, dtype=torch.float32, device=dev) if vote and probs else None,
                    torch.empty(n, k, dtype=torch.int32, device=dev) if neighbours else None,
                    torch.empty(n, k, dtype=torch.float32, device=dev) if neighbours else None)
    _lib.check("cmlpl_knn", _lib.load().cmlpl_knn(
        query.data_ptr(), n, gallery.data_ptr(), m, _lib.ptr(gallery_labels), K, _lib.ptr(skip), int(k),
        inv_T_of(T) if vote else 1.0, _lib.ptr(res.nbr_idx), _lib.ptr(res.nbr_sim), _lib.ptr(res.probs), _lib.ptr(res.labels),
        workspace.data_ptr(), workspace.numel(), _lib.stream(dev)))
    return res


class KnnEvaluator:
    """``KnnEvaluator(shape, gallery_spectra, gallery_labels, query_spectra, query_truth, k, T, loo=False)``: the gallery
    (spectra float32 cuda [m, bands], labels int64 cuda [m]) and the query list (spectra [n, bands], truth int64 [n];
    outside 0 .. K - 1 = unlabelled, counted in no matrix) are registered once, with every buffer an evaluation needs.
    ``loo``: leave-one-out -- the queries ARE the gallery (``query_spectra`` / ``query_truth`` may be None) and query i
    skips gallery row i.  No cube: the embedding is spectral.  ``evaluate`` is launches only and synchronises nothing."""

    def __init__(self, shape, gallery_spectra, gallery_labels, query_spectra=None, query_truth=None, k: int = 10,
                 T: float = 0.07, loo: bool = False, neighbours: bool = False):
        import torch
        from . import _lib
        self.lib = _lib.load()
        self.shape, self.k, self.T, self.loo, self.neighbours = shape, int(k), float(T), bool(loo), bool(neighbours)
        inv_T_of(T)
        if loo:
            if query_spectra is None:
                query_spectra, query_truth = gallery_spectra, gallery_labels
            elif query_spectra is not gallery_spectra or query_truth is not gallery_labels:
                raise ValueError("loo: the queries are the gallery")
        for t, name in ((gallery_spectra, "gallery_spectra"), (query_spectra, "query_spectra")):
            if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.shape[1] == shape.bands
                    and t.shape[0] >= 1):
                raise ValueError(f"{name}: need a contiguous float32 cuda tensor [., {shape.bands}]")
        dev = gallery_spectra.device
        self.m, self.n = gallery_spectra.shape[0], query_spectra.shape[0]
        _list_ok(gallery_labels, self.m, "gallery_labels", dev)
        _list_ok(query_truth, self.n, "query_truth", dev)
        if not 1 <= shape.K <= K_MAX or not 1 <= self.k <= NBR_MAX:
            raise ValueError("K: 1 .. 64, k: 1 .. 32")
        self.gallery_spectra, self.gallery_labels = gallery_spectra, gallery_labels
        self.query_spectra, self.truth = query_spectra, query_truth
        self.skip = torch.arange(self.n, dtype=torch.int64, device=dev) if loo else None
        K = shape.K
        self.gfeat = torch.empty(2, self.m, D, dtype=torch.float32, device=dev)
        self.gnorm = torch.empty(2, self.m, dtype=torch.float32, device=dev)
        self.qfeat = self.gfeat if loo else torch.empty(2, self.n, D, dtype=torch.float32, device=dev)
        self.qnorm = self.gnorm if loo else torch.empty(2, self.n, dtype=torch.float32, device=dev)
        self.labels = torch.empty(2, self.n, dtype=torch.int64, device=dev)
        self.probs = torch.empty(2, self.n, K, dtype=torch.float32, device=dev)
        self.nbr_idx = torch.empty(2, self.n, self.k, dtype=torch.int32, device=dev) if neighbours else None
        self.nbr_sim = torch.empty(2, self.n, self.k, dtype=torch.float32, device=dev) if neighbours else None
        self.ws = torch.empty(workspace_bytes(self.n, self.m, self.k), dtype=torch.uint8, device=dev)
        self.cm = torch.zeros(2, K, K, dtype=torch.int64, device=dev)
        self.ignored = torch.zeros(1, dtype=torch.int64, device=dev)
        self.last = None

    def evaluate(self, nets):
        """confusion matrices int64 [nets, K, K] on the device (row = true class, column = the vote's label; a query
        without a candidate is in no column) of the registered queries under ``nets`` (see ``embed``).  A view of this
        object's buffer: the next call overwrites it.  ``.last``: the ``KnnResult`` with a leading network dimension
        ([nets, n], [nets, n, K], ..); ``cmlpl_amd.calibrate.reliability(ev.last.probs[j], ev.truth)`` scores network j."""
        import torch
        from . import _lib
        from .infer import _nets_buffers
        with torch.no_grad():
            cs, nn = _nets_buffers(nets)[:2]
            if (cs.C, cs.H, cs.W, cs.bands, cs.K) != (self.shape.C, self.shape.H, self.shape.W, self.shape.bands, self.shape.K):
                raise ValueError("the networks' shape is not the registered one")
            n, m, K, k = self.n, self.m, self.shape.K, self.k
            embed(nets, self.gallery_spectra, out=(self.gfeat[:nn], self.gnorm[:nn]))
            if not self.loo:
                embed(nets, self.query_spectra, out=(self.qfeat[:nn], self.qnorm[:nn]))
            dev = self.gfeat.device
            inv = inv_T_of(self.T)
            for j in range(nn):
                res = KnnResult(self.labels[j], self.probs[j], None if self.nbr_idx is None else self.nbr_idx[j],
                                None if self.nbr_sim is None else self.nbr_sim[j])
                _lib.check("cmlpl_knn", self.lib.cmlpl_knn(
                    self.qfeat[j].data_ptr(), n, self.gfeat[j].data_ptr(), m, self.gallery_labels.data_ptr(), K,
                    _lib.ptr(self.skip), k, inv, _lib.ptr(res.nbr_idx), _lib.ptr(res.nbr_sim), res.probs.data_ptr(),
                    res.labels.data_ptr(), self.ws.data_ptr(), self.ws.numel(), _lib.stream(dev)))
            self.last = KnnResult(self.labels[:nn], self.probs[:nn], None if self.nbr_idx is None else self.nbr_idx[:nn],
                                  None if self.nbr_sim is None else self.nbr_sim[:nn])
            cm = self.cm[:nn]
            cm.zero_()
            self.ignored.zero_()
            _lib.check("cmlpl_confusion", self.lib.cmlpl_confusion(
                self.labels.data_ptr(), nn, self.truth.data_ptr(), n, K, cm.data_ptr(), self.ignored.data_ptr(), _lib.stream(dev)))
            return cm
