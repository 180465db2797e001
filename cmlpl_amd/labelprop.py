"""Label propagation over the embedding's kNN graph: build, diffuse, score (include/cmlpl.h, "THE DEFINITION OF A PROPAGATED
LABELLING").

A kNN vote (cmlpl_amd.knn) reaches as far as a seed's own neighbourhood.  Label propagation -- the "label spreading" of Zhou
et al. (NIPS 2003), as Iscen et al. (CVPR 2019) use it on deep embeddings -- also uses how the UNLABELLED rows lie between
the seeds: the rows are the nodes of the symmetrised kNN graph W = A + A^T, and F <- alpha S F + (1 - alpha) Y is iterated
over S = D^-1/2 W D^-1/2.  ``knn_graph`` is the existing search alone (leave-one-out), ``build_graph`` turns its lists into
the graph workspace (``cmlpl_lp_graph``, csrc/labelprop.hip), ``propagate`` iterates and scores (``cmlpl_lp_propagate``),
``label_propagation`` is the three in one call.  ``labelprop_host`` restates the definition in numpy, list order included:
it touches no GPU, and the tests hold the kernels to it."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

K_MAX, NBR_MAX, GAMMA_MAX, ITERS_MAX = 64, 32, 8, 10000


class LabelProp(NamedTuple):
    """the configuration of ``label_propagation``.  The defaults are NOT tuned: they are the values commonly quoted for the
    method (Iscen et al. use gamma = 3 and alpha = 0.99), not the result of a search on any scene."""
    k: int = 10
    alpha: float = 0.99
    gamma: int = 3
    iters: int = 50

    def check(self):
        if not 1 <= int(self.k) <= NBR_MAX:
            raise ValueError("k: 1 .. 32 neighbours")
        if not (0.0 <= float(self.alpha) < 1.0):
            raise ValueError("alpha: 0 <= alpha < 1")
        if not 1 <= int(self.gamma) <= GAMMA_MAX:
            raise ValueError("gamma: an integer 1 .. 8")
        if not 1 <= int(self.iters) <= ITERS_MAX:
            raise ValueError("iters: 1 .. 10000")
        return self


class LPResult(NamedTuple):
    """what ``propagate`` returns; a field that was not asked for is None"""
    labels: object          # int64 [n]: the first maximum of probs, -1 for an unreached node
    probs: object           # float32 [n, K]: F / its row sum (a NaN row for an unreached node)
    conf: object            # float32 [n]: probs[label]
    entropy: object         # float32 [n]
    F: object               # float32 [n, K]: the iterate itself (pass it as F0 to go on)
    residual: object        # float32 [1]: max |F_T - F_{T-1}|


class LPGraph:
    """the graph workspace of ``cmlpl_lp_graph`` and views of its arrays (include/cmlpl.h, "THE GRAPH WORKSPACE")"""

    def __init__(self, buf, n: int, k: int):
        import torch
        self.buf, self.n, self.k = buf, int(n), int(k)
        n, N = self.n, self.n * self.k
        words = buf[:4 * (3 * n + 1 + 5 * N)]
        f, i = words.view(torch.float32), words.view(torch.int32)
        o = 0
        self.cinv = f[o:o + n]; o += n
        self.fwd_coef = f[o:o + N].view(n, self.k); o += N
        self.rev_ptr = i[o:o + n + 1]; o += n + 1
        self.rev_src = i[o:o + N]; o += N
        self.rev_coef = f[o:o + N]; o += N
        self.fwd_dst = i[o:o + N].view(n, self.k); o += N
        self.rev_edge = i[o:o + N]; o += N
        self.in_deg = i[o:o + n]

    def edges(self) -> int:
        """the number of directed entries that are edges (every one appears once forward and once reversed); synchronises"""
        return int(self.rev_ptr[self.n])

    def max_in_degree(self) -> int:
        """the longest reverse list; synchronises"""
        return int(self.in_deg.max())


def knn_graph(feat, k: int):
    """(nbr_idx int32 [n, k], nbr_sim float32 [n, k]) of the rows of ``feat`` [n, 1024] among themselves: the existing search
    alone (``cmlpl_amd.knn.knn`` without labels) with ``skip = arange(n)``"""
    import torch
    from .knn import knn
    n = feat.shape[0]
    res = knn(feat, feat, None, 0, int(k), skip=torch.arange(n, dtype=torch.int64, device=feat.device))
    return res.nbr_idx, res.nbr_sim


def graph_bytes(n: int, k: int) -> int:
    from . import _lib
    need = _lib.load().cmlpl_lp_graph_bytes(int(n), int(k))
    if need == 0:
        raise ValueError("label propagation: n >= 1, 1 <= k <= 32, n k < 2^31")
    return need


def build_graph(nbr_idx, nbr_sim, gamma: int = 3) -> LPGraph:
    """the symmetrised, normalised graph of neighbour lists int32 / float32 cuda [n, k] as ``cmlpl_knn`` writes them.
    Launches on the current stream, no synchronisation."""
    import torch
    from . import _lib
    if not (nbr_idx.is_cuda and nbr_idx.dtype == torch.int32 and nbr_idx.dim() == 2 and nbr_idx.is_contiguous()):
        raise ValueError("nbr_idx: a contiguous int32 cuda tensor [n, k]")
    if not (nbr_sim.is_cuda and nbr_sim.dtype == torch.float32 and nbr_sim.shape == nbr_idx.shape and nbr_sim.is_contiguous()
            and nbr_sim.device == nbr_idx.device):
        raise ValueError("nbr_sim: a contiguous float32 cuda tensor of nbr_idx's shape on its device")
    n, k = nbr_idx.shape
    if not 1 <= int(gamma) <= GAMMA_MAX:
        raise ValueError("gamma: an integer 1 .. 8")
    buf = torch.empty(graph_bytes(n, k), dtype=torch.uint8, device=nbr_idx.device)
    _lib.check("cmlpl_lp_graph", _lib.load().cmlpl_lp_graph(nbr_idx.data_ptr(), nbr_sim.data_ptr(), n, k, int(gamma),
                                                            buf.data_ptr(), buf.numel(), _lib.stream(buf.device)))
    return LPGraph(buf, n, k)


def one_hot_seeds(labels, K: int):
    """Y float32 [n, K] of int64 labels [n]: a one-hot row per seed, a zero row for anything outside 0 .. K - 1"""
    import torch
    if labels.dtype != torch.int64 or labels.dim() != 1:
        raise ValueError("labels: an int64 vector")
    ok = (labels >= 0) & (labels < K)
    Y = torch.zeros(labels.shape[0], K, dtype=torch.float32, device=labels.device)
    Y.scatter_(1, torch.where(ok, labels, torch.zeros_like(labels)).unsqueeze(1), ok.to(torch.float32).unsqueeze(1))
    return Y


def propagate(graph: LPGraph, Y, alpha: float, iters: int, F0=None, probs: bool = True, conf: bool = False,
              entropy: bool = False, residual: bool = False) -> LPResult:
    """``iters`` iterations F <- alpha S F + (1 - alpha) Y over ``graph`` from ``F0`` (None: Y), and the finish: labels always,
    ``probs`` / ``conf`` / ``entropy`` / ``residual`` when asked for.  Y float32 cuda [n, K], non-negative, is only read.
    Launches on the current stream and does not synchronise."""
    import torch
    from . import _lib
    n = graph.n
    dev = graph.buf.device
    for t, name in ((Y, "Y"), (F0, "F0")):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.shape[0] == n
                                  and t.device == dev and t.shape[1] == Y.shape[1]):
            raise ValueError(f"{name}: a contiguous float32 cuda tensor [{n}, K] on the graph's device")
    K = Y.shape[1]
    if not 1 <= K <= K_MAX:
        raise ValueError("K: 1 .. 64")
    alpha = float(alpha)
    if not (0.0 <= alpha < 1.0) or not (0.0 <= float(np.float32(alpha)) < 1.0):
        raise ValueError("alpha: 0 <= alpha < 1")
    if not 1 <= int(iters) <= ITERS_MAX:
        raise ValueError("iters: 1 .. 10000")
    new = lambda *shape, dt=torch.float32: torch.empty(*shape, dtype=dt, device=dev)
    res = LPResult(new(n, dt=torch.int64), new(n, K) if probs else None, new(n) if conf else None, new(n) if entropy else None,
                   new(n, K), new(1) if residual else None)
    tmp = new(n, K)
    _lib.check("cmlpl_lp_propagate", _lib.load().cmlpl_lp_propagate(
        graph.buf.data_ptr(), n, graph.k, Y.data_ptr(), K, alpha, int(iters), _lib.ptr(F0), res.F.data_ptr(), tmp.data_ptr(),
        _lib.ptr(res.probs), res.labels.data_ptr(), _lib.ptr(res.conf), _lib.ptr(res.entropy), _lib.ptr(res.residual),
        _lib.stream(dev)))
    return res


def label_propagation(feat, seed_labels, K: int, cfg: LabelProp = LabelProp(), **outputs) -> LPResult:
    """the three steps in one call: the kNN graph of ``feat`` [n, 1024] (float32 cuda, unit rows), the graph workspace, the
    propagation of ``one_hot_seeds(seed_labels, K)`` (int64 cuda [n]; outside 0 .. K - 1 = no seed).  ``outputs``: the
    keywords of ``propagate``."""
    cfg = LabelProp(*cfg).check()
    idx, sim = knn_graph(feat, cfg.k)
    return propagate(build_graph(idx, sim, cfg.gamma), one_hot_seeds(seed_labels, K), cfg.alpha, cfg.iters, **outputs)


def propagate_embedding(nets, spectra, seed_labels, K: int, cfg: LabelProp = LabelProp(), **outputs):
    """``label_propagation`` on the embedding (``cmlpl_amd.knn.embed``) of the node spectra float32 cuda [n, bands] under every
    network of ``nets`` (what ``embed`` takes): a list of (LPGraph, LPResult), one pair per network.  A dead-ReLU row has a
    NaN embedding, is nobody's neighbour and stays unreached unless it is a seed."""
    from .knn import embed
    cfg = LabelProp(*cfg).check()
    feat = embed(nets, spectra)[0]
    Y = one_hot_seeds(seed_labels, K)
    out = []
    for f in (feat if feat.dim() == 3 else feat.unsqueeze(0)):
        graph = build_graph(*knn_graph(f, cfg.k), cfg.gamma)
        out.append((graph, propagate(graph, Y, cfg.alpha, cfg.iters, **outputs)))
    return out


def score_labels(labels, truth, K: int):
    """(OA, Kappa, producerA, AA, matrix) of propagated labels against int truths 0 .. K - 1: the confusion matrix int64
    [K, K + 1] has a last column for the UNREACHED rows (label -1), which so count as wrong for their class"""
    labels, truth = np.asarray(labels, np.int64), np.asarray(truth, np.int64)
    keep = (truth >= 0) & (truth < K)
    cm = np.zeros((K, K + 1), np.int64)
    np.add.at(cm, (truth[keep], np.where(labels[keep] < 0, K, labels[keep])), 1)
    n = int(truth[keep].max()) + 1 if keep.any() else 1        # (classes past the last one present are left out, as CalAccuracy does)
    c = cm[:n].astype(np.float64)
    total = max(c.sum(), 1.0)
    OA = np.trace(c[:, :n]) / total
    pe = float((c[:, :n].sum(0) * c.sum(1)).sum()) / (total * total)
    Kappa = (OA - pe) / (1.0 - pe) if pe < 1.0 else 0.0
    producerA = np.diag(c[:, :n]) / np.maximum(c.sum(1), 1.0)
    return OA, Kappa, producerA, float(np.mean(producerA)), cm


# ------------------------------------------------------------------ the definition, restated in numpy
class LPHost(NamedTuple):
    rev_ptr: np.ndarray     # int32 [n + 1]
    rev_src: np.ndarray     # int32 [E]
    cinv: np.ndarray        # dtype [n]
    fwd_coef: np.ndarray    # dtype [n, k]
    rev_coef: np.ndarray    # dtype [E]
    F: np.ndarray           # dtype [n, K]
    probs: np.ndarray       # dtype [n, K]
    labels: np.ndarray      # int64 [n]
    conf: np.ndarray        # dtype [n]
    entropy: np.ndarray     # dtype [n]
    residual: float


def _by_position(owner, start, length):
    """the slots of ragged lists grouped by their position in the list: for pos = 0, 1, .. the array of slots that stand at
    that position of their owner's list (slots are list-major, ``start[owner]`` + position)"""
    pos = np.arange(len(owner), dtype=np.int64) - start[owner]
    order = np.argsort(pos, kind="stable")
    cuts = np.searchsorted(pos[order], np.arange(int(length.max(initial=0)) + 1))
    return [order[cuts[p]:cuts[p + 1]] for p in range(len(cuts) - 1)]


def labelprop_host(nbr_idx, nbr_sim, Y, alpha: float, gamma: int, iters: int, F0=None, dtype=np.float64) -> LPHost:
    """The definition in numpy, list order included.  ``dtype=np.float32`` evaluates the same chain in fp32 (every operation
    rounded on its own: no FMA); the similarities are taken as fl32 either way, as the device reads them."""
    dt = np.dtype(dtype).type
    idx = np.asarray(nbr_idx, np.int64)
    n, k = idx.shape
    sim32 = np.asarray(nbr_sim, np.float32)
    Y = np.asarray(Y, np.float32).astype(dt)
    K = Y.shape[1]
    if not (1 <= k <= NBR_MAX and 1 <= K <= K_MAX and 1 <= gamma <= GAMMA_MAX and 1 <= iters <= ITERS_MAX and 0.0 <= alpha < 1.0):
        raise ValueError("labelprop_host: an argument outside the definition's ranges")
    alpha32 = np.float32(alpha)
    beta = dt(np.float32(1.0 - float(alpha32)))
    al = dt(alpha32)
    node = np.repeat(np.arange(n, dtype=np.int64), k)
    flat = idx.reshape(-1)
    edge = (flat >= 0) & (flat != node)
    with np.errstate(all="ignore"):
        s = sim32.reshape(-1)
        pos_s = (s > 0) & (s <= np.finfo(np.float32).max)
        base = np.where(pos_s, s, np.float32(0)).astype(dt)
        a = base.copy()
        for _ in range(gamma - 1):
            a = (a * base).astype(dt)
    a = np.where(edge, a, dt(0))
    # the reverse lists: the entries e = j k + r that are edges, stably sorted by their target: (j, r) ascending inside a target
    ids = np.nonzero(edge)[0]
    order = ids[np.argsort(flat[ids], kind="stable")]
    tgt = flat[order]
    rev_src = node[order].astype(np.int32)
    in_deg = np.bincount(tgt, minlength=n).astype(np.int64)
    rev_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(in_deg, out=rev_ptr[1:])
    rev_w = a[order]
    # degrees: one chain in list order, forward then reverse
    d = np.zeros(n, dt)
    for r in range(k):
        e = np.arange(n) * k + r
        d = np.where(edge[e], (d + a[e]).astype(dt), d)
    rev_groups = _by_position(tgt, rev_ptr[:-1], in_deg)
    for slots in rev_groups:
        d[tgt[slots]] = (d[tgt[slots]] + rev_w[slots]).astype(dt)
    with np.errstate(all="ignore"):
        cinv = np.where(d > 0, (dt(1) / np.sqrt(d).astype(dt)).astype(dt), dt(0))
    safe = np.where(edge, flat, 0)
    fwd_coef = np.where(edge, ((cinv[node] * a).astype(dt) * cinv[safe]).astype(dt), dt(0)).reshape(n, k)
    rev_coef = ((cinv[tgt] * rev_w).astype(dt) * cinv[rev_src]).astype(dt)
    fwd_rows = [np.nonzero(edge.reshape(n, k)[:, r])[0] for r in range(k)]
    F = Y.copy() if F0 is None else np.asarray(F0, np.float32).astype(dt)
    prev = F
    with np.errstate(all="ignore"):
        for _ in range(iters):
            acc = np.zeros((n, K), dt)
            for r in range(k):
                rows = fwd_rows[r]
                acc[rows] = (acc[rows] + (fwd_coef[rows, r, None] * F[idx[rows, r]]).astype(dt)).astype(dt)
            for slots in rev_groups:
                rows = tgt[slots]
                acc[rows] = (acc[rows] + (rev_coef[slots, None] * F[rev_src[slots]]).astype(dt)).astype(dt)
            prev, F = F, ((al * acc).astype(dt) + (beta * Y).astype(dt)).astype(dt)
        diff = np.abs(F - prev)
        residual = float("nan") if np.isnan(diff).any() else float(diff.max())
        z = np.zeros(n, dt)
        for c in range(K):
            z = (z + F[:, c]).astype(dt)
        ok = z > 0
        p = np.where(ok[:, None], (F / np.where(ok, z, dt(1))[:, None]).astype(dt), dt(np.nan))
        labels = np.where(ok, np.where(ok[:, None], p, dt(0)).argmax(1), -1).astype(np.int64)
        conf = np.where(ok, np.take_along_axis(np.where(ok[:, None], p, dt(0)), np.maximum(labels, 0)[:, None], 1)[:, 0], dt(np.nan))
        h = np.zeros(n, dt)
        for c in range(K):
            pc = p[:, c]
            term = np.where(pc > 0, (pc * np.log(np.where(pc > 0, pc, dt(1))).astype(dt)).astype(dt), dt(0))
            h = (h + term).astype(dt)
        entropy = np.where(ok, -h, dt(np.nan))
    return LPHost(rev_ptr.astype(np.int32), rev_src, cinv, fwd_coef, rev_coef, F, p, labels, conf, entropy, residual)
