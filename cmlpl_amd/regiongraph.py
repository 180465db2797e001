"""The region graph: superpixels (or any regions) as the nodes of a label propagation, and a whole-scene map from it
(``cmlpl_rg_pool`` / ``cmlpl_rg_adjacency`` / ``cmlpl_rg_lists``, csrc/regiongraph.hip; the reference has no counterpart).

The region vote (cmlpl_amd.superpixel) lets every region decide alone; label propagation (cmlpl_amd.labelprop) diffuses over a
kNN graph, but a pixel graph of a whole scene is 207,400 nodes of 1,024 floats.  A region graph of the same scene has 1,000 to
13,000 nodes: ``pool`` gives every region of an int32 map its mean spectrum, ``adjacency`` its 4-connected neighbours by
shared boundary length, ``merge_lists`` joins the kNN lists of the regions' embeddings with them into the lists
``build_graph`` takes, and the vote becomes the prior Y of a diffusion over similar and adjacent regions -- superpixel-graph
regularisation, the usual last step of object-based hyperspectral classification.  The definitions are in ``include/cmlpl.h``
("THE DEFINITION OF A REGION DESCRIPTOR", "... OF A REGION ADJACENCY", "... OF A REGION GRAPH"); ``pool_host``,
``adjacency_host``, ``merge_lists_host`` and ``region_graph_host`` restate them in numpy and touch no GPU.

Not built: seeds from the command line, per-member graphs averaged, 8-connected adjacency, edge weights from the boundary
length, a sharded version.  Nothing here synchronises; everything runs on the current stream."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from .labelprop import GAMMA_MAX, ITERS_MAX, NBR_MAX

A_MAX, B_MAX, D = 16, 1024, 1024
N_MAX = 1 << 27
POOL_MAX = 256.0
FIX24 = 16777216.0


class RegionGraph(NamedTuple):
    """``k`` kNN neighbours in the embedding of member ``net`` and the ``adj`` spatial neighbours of the longest shared
    boundary per region (1 <= k + adj <= 32, adj <= 16), then ``iters`` iterations F <- alpha S F + (1 - alpha) Y at ``gamma``.
    The defaults are NOT tuned on any scene: a moderate alpha keeps a region's own vote the larger share."""
    k: int = 8
    adj: int = 8
    alpha: float = 0.5
    gamma: int = 3
    iters: int = 20
    net: int = 0

    def check(self, members: Optional[int] = None):
        k, A = int(self.k), int(self.adj)
        if k < 0 or not 0 <= A <= A_MAX or not 1 <= k + A <= NBR_MAX:
            raise ValueError(f"RegionGraph: k >= 0, adj 0 .. {A_MAX}, k + adj 1 .. {NBR_MAX}")
        if not (0.0 <= float(self.alpha) < 1.0) or not (0.0 <= float(np.float32(self.alpha)) < 1.0):
            raise ValueError("RegionGraph: 0 <= alpha < 1")
        if not 1 <= int(self.gamma) <= GAMMA_MAX:
            raise ValueError(f"RegionGraph: gamma an integer 1 .. {GAMMA_MAX}")
        if not 1 <= int(self.iters) <= ITERS_MAX:
            raise ValueError(f"RegionGraph: iters 1 .. {ITERS_MAX}")
        if int(self.net) < 0 or (members is not None and int(self.net) >= members):
            raise ValueError("RegionGraph: net names no member")
        return self


class Pooled(NamedTuple):
    mean: object            # float32 [M, B]: the mean of the region's pooled pixels (a zero row: none)
    cnt: object             # int64 [M]: its pooled pixels
    S: object = None        # int64 [M, B]: the fixed-point sums (when asked for)


class Adjacency(NamedTuple):
    adj_idx: object         # int32 [M, A]: the neighbours by (boundary length descending, id ascending), -1 past the end
    adj_len: object         # int32 [M, A]: their shared boundary lengths, 0 past the end
    deg: object             # int32 [M]: the regions it touches
    boundary: object        # int32 [M]: the sum of its boundary lengths


class RegionGraphResult(NamedTuple):
    graph: object           # the LPGraph of the regions
    ids: object             # int32 [n]: the map
    M: int
    pooled: Pooled
    feat: object            # float32 [M, 1024]: the embedding of the mean spectra (a NaN row: an empty region)
    adjacency: Adjacency
    nbr_idx: object         # int32 [M, k + adj]
    nbr_sim: object         # float32 [M, k + adj]


class RegionPropagated(NamedTuple):
    """the leading four fields of every result tuple, per pixel, and the per-region ``LPResult`` behind them"""
    labels: object                      # int64 [n]; -1: a void pixel, or a pixel of an unreached region
    probs: object = None                # float32 [n, K]
    conf: object = None                 # float32 [n]
    entropy: object = None              # float32 [n]
    regions: object = None              # LPResult over the M regions
    Y: object = None                    # float32 [M, K]: what was propagated


def _map_ok(ids, M, n=None):
    import torch
    if not (torch.is_tensor(ids) and ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous()
            and 1 <= ids.shape[0] <= N_MAX and (n is None or ids.shape[0] == n)):
        raise ValueError("ids: need a contiguous int32 cuda tensor [rows * cols], at most 2^27 pixels")
    if not 1 <= int(M) <= N_MAX:
        raise ValueError("M: 1 .. 2^27 regions")
    return int(M)


def _workspace(lib, rows, cols, M, A, dev):
    import torch
    nbytes = lib.cmlpl_rg_workspace_bytes(rows, cols, M, A)
    if nbytes == 0:
        raise ValueError("region graph: rows, cols, M >= 1, at most 2^27 pixels and regions, A 0 .. 16")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def pool(ids, M: int, X, sums: bool = False) -> Pooled:
    """the descriptor of every region of the int32 cuda map ``ids`` [n] (outside 0 .. M - 1: void) from ``X`` float32 cuda
    [n, B] (1 <= B <= 1024; rows of unit stride, any row stride >= B): a pixel with a value that is not finite or beyond
    +-256 is left out whole.  ``sums``: also the int64 fixed-point sums."""
    import torch
    from . import _lib
    M = _map_ok(ids, M)
    n = ids.shape[0]
    if not (torch.is_tensor(X) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.shape[0] == n
            and 1 <= X.shape[1] <= B_MAX and X.stride(1) == 1 and X.stride(0) >= X.shape[1] and X.device == ids.device):
        raise ValueError(f"X: need a float32 cuda tensor [n, B], 1 <= B <= {B_MAX}, unit stride along B, on the map's device")
    lib, dev, B = _lib.load(), ids.device, X.shape[1]
    res = Pooled(torch.empty(M, B, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.int64, device=dev),
                 torch.empty(M, B, dtype=torch.int64, device=dev) if sums else None)
    ws, nbytes = _workspace(lib, 1, n, M, 0, dev)
    _lib.check("cmlpl_rg_pool", lib.cmlpl_rg_pool(ids.data_ptr(), 1, n, M, X.data_ptr(), X.stride(0), B, res.mean.data_ptr(),
                                                  res.cnt.data_ptr(), _lib.ptr(res.S), ws.data_ptr(), nbytes, _lib.stream(dev)))
    return res


def adjacency(ids, M: int, rows: int, cols: int, A: int) -> Adjacency:
    """the 4-connected neighbours of every region of the map ``ids`` [rows * cols]: the ``A`` (0 .. 16) of the longest
    shared boundary, ties to the smaller id; ``deg`` and ``boundary`` count all of them"""
    import torch
    from . import _lib
    rows, cols, A = int(rows), int(cols), int(A)
    if rows < 1 or cols < 1:
        raise ValueError("adjacency: rows, cols >= 1")
    M = _map_ok(ids, M, rows * cols)
    if not 0 <= A <= A_MAX:
        raise ValueError(f"adjacency: A 0 .. {A_MAX}")
    lib, dev = _lib.load(), ids.device
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    res = Adjacency(i32(M, A), i32(M, A), i32(M), i32(M))
    ws, nbytes = _workspace(lib, rows, cols, M, A, dev)
    _lib.check("cmlpl_rg_adjacency", lib.cmlpl_rg_adjacency(
        ids.data_ptr(), rows, cols, M, A, res.adj_idx.data_ptr() if A else None, res.adj_len.data_ptr() if A else None,
        res.deg.data_ptr(), res.boundary.data_ptr(), ws.data_ptr(), nbytes, _lib.stream(dev)))
    return res


def merge_lists(feat, knn_idx, knn_sim, adj_idx):
    """(nbr_idx int32, nbr_sim float32) [M, k + A]: the kNN lists [M, k] (None: k = 0) copied, then per adjacent region that is
    no kNN neighbour already the fp32 dot product of the two rows of ``feat`` [M, 1024]; -1 / -inf elsewhere"""
    import torch
    from . import _lib
    if not (torch.is_tensor(feat) and feat.is_cuda and feat.dtype == torch.float32 and feat.dim() == 2 and feat.shape[1] == D
            and feat.is_contiguous() and 1 <= feat.shape[0] <= N_MAX):
        raise ValueError(f"feat: need a contiguous float32 cuda tensor [M, {D}]")
    M, dev = feat.shape[0], feat.device
    k = 0 if knn_idx is None else knn_idx.shape[1] if knn_idx.dim() == 2 else -1
    if (knn_idx is None) != (knn_sim is None) or k < 0:
        raise ValueError("knn_idx / knn_sim: both [M, k], or both None")
    for t, dt, name in ((knn_idx, torch.int32, "knn_idx"), (knn_sim, torch.float32, "knn_sim"), (adj_idx, torch.int32, "adj_idx")):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.dim() == 2 and t.shape[0] == M and t.is_contiguous()
                                  and t.device == dev and (name == "adj_idx" or t.shape[1] == k)):
            raise ValueError(f"{name}: need a contiguous {dt} cuda tensor [M, .] on feat's device")
    A = 0 if adj_idx is None else adj_idx.shape[1]
    if not (A <= A_MAX and 1 <= k + A <= NBR_MAX):
        raise ValueError(f"merge_lists: A 0 .. {A_MAX}, k + A 1 .. {NBR_MAX}")
    nbr_idx = torch.empty(M, k + A, dtype=torch.int32, device=dev)
    nbr_sim = torch.empty(M, k + A, dtype=torch.float32, device=dev)
    _lib.check("cmlpl_rg_lists", _lib.load().cmlpl_rg_lists(
        feat.data_ptr(), M, knn_idx.data_ptr() if k else None, knn_sim.data_ptr() if k else None, k,
        adj_idx.data_ptr() if A else None, A, nbr_idx.data_ptr(), nbr_sim.data_ptr(), _lib.stream(dev)))
    return nbr_idx, nbr_sim


def region_graph(ids, M: int, rows: int, cols: int, spectra, nets, cfg: RegionGraph = RegionGraph()) -> RegionGraphResult:
    """the graph of the regions of ``ids`` [rows * cols]: pool of ``spectra`` [n, bands]; the embedding (cmlpl_amd.knn.embed)
    of the mean spectra under member ``cfg.net`` of ``nets`` (a list of members, or one: a module, or (engine, index));
    the rows of empty regions set to NaN, so nobody takes them as a neighbour; their kNN lists (leave-one-out) unless
    k == 0; the adjacency; the merged lists; ``build_graph``.  Launches only."""
    import torch
    from .knn import embed, knn
    from .labelprop import build_graph
    members = list(nets) if isinstance(nets, list) else [nets]
    cfg = RegionGraph(*cfg).check(len(members))
    pooled = pool(ids, M, spectra)
    feat = embed(members[int(cfg.net)], pooled.mean)[0]
    if feat.dim() != 2:
        raise ValueError("region_graph: a member is ONE network (a module, or (engine, index))")
    feat = torch.where((pooled.cnt == 0).unsqueeze(1), torch.full_like(feat, float("nan")), feat)
    k, A = int(cfg.k), int(cfg.adj)
    knn_idx = knn_sim = None
    if k > 0:
        res = knn(feat, feat, None, 0, k, skip=torch.arange(M, dtype=torch.int64, device=feat.device))
        knn_idx, knn_sim = res.nbr_idx, res.nbr_sim
    adj = adjacency(ids, M, rows, cols, A)
    nbr_idx, nbr_sim = merge_lists(feat, knn_idx, knn_sim, adj.adj_idx if A else None)
    return RegionGraphResult(build_graph(nbr_idx, nbr_sim, int(cfg.gamma)), ids, int(M), pooled, feat, adj, nbr_idx, nbr_sim)


def region_prior(q, ids=None, M=None, seeds=None):
    """Y float32 [M, K] of the region vote's ``q`` (its ``seg_probs``): a NaN row becomes a zero row; with ``seeds`` = (pix,
    labels) the row of every region that holds a seed is REPLACED by the normalised class histogram of its seeds (the hard
    vote of those pixels over the map, as ``asa`` builds it)"""
    import torch
    from .superpixel import region_vote
    Y = torch.where(torch.isnan(q), torch.zeros_like(q), q).contiguous()
    if seeds is not None:
        pix, labels = (torch.as_tensor(np.asarray(v, np.int64) if not torch.is_tensor(v) else v).to(ids.device).long() for v in seeds)
        tm = torch.full((ids.shape[0],), -1, dtype=torch.int64, device=ids.device)
        tm[pix] = labels
        vote = region_vote(ids, labels=tm, K=q.shape[1], N=int(M), probs_out=False)
        Y = torch.where((vote.seg_counts > 0).unsqueeze(1), vote.seg_probs, Y).contiguous()
    return Y


def region_propagate(rg: RegionGraphResult, q, cfg: RegionGraph = RegionGraph(), seeds=None, probs_out: bool = True,
                     conf: bool = False, entropy: bool = False) -> RegionPropagated:
    """``propagate`` of ``region_prior(q, seeds)`` over ``rg.graph``, then every pixel of region s takes the label,
    probabilities, confidence and entropy of s; a void pixel and a pixel of an unreached region get -1 and NaN"""
    import torch
    from .labelprop import propagate
    cfg = RegionGraph(*cfg).check()
    if not (torch.is_tensor(q) and q.is_cuda and q.dtype == torch.float32 and q.dim() == 2 and q.shape[0] == rg.M):
        raise ValueError("q: need a float32 cuda tensor [M, K], the region vote's seg_probs")
    Y = region_prior(q, rg.ids, rg.M, seeds)
    res = propagate(rg.graph, Y, float(cfg.alpha), int(cfg.iters), probs=probs_out, conf=conf, entropy=entropy, residual=True)
    ids = rg.ids.long()
    inside = (ids >= 0) & (ids < rg.M)
    at = torch.where(inside, ids, torch.zeros_like(ids))
    nan = float("nan")
    labels = torch.where(inside, res.labels[at], torch.full_like(ids, -1))
    take = lambda v: None if v is None else torch.where(inside if v.dim() == 1 else inside.unsqueeze(1), v[at], torch.full_like(v[at], nan))
    return RegionPropagated(labels, take(res.probs), take(res.conf), take(res.entropy), res, Y)


# ------------------------------------------------------------------ the definitions, in numpy
def pool_host(ids, M: int, X) -> dict:
    """THE DEFINITION OF A REGION DESCRIPTOR: dict(S int64 [M, B], cnt int64 [M], mean float32 [M, B])"""
    ids, X, M = np.asarray(ids, np.int64).reshape(-1), np.asarray(X, np.float32), int(M)
    B = X.shape[1]
    with np.errstate(invalid="ignore"):
        pooled = (ids >= 0) & (ids < M) & (np.isfinite(X) & (np.abs(X) <= np.float32(POOL_MAX))).all(1)
    S = np.zeros((M, B), np.int64)
    np.add.at(S, ids[pooled], np.rint(X[pooled].astype(np.float64) * FIX24).astype(np.int64))     # llrintf(x * 2^24): exact product
    cnt = np.bincount(ids[pooled], minlength=M).astype(np.int64)
    mean = np.zeros((M, B), np.float32)
    has = cnt > 0
    mean[has] = (S[has].astype(np.float64) / (cnt[has].astype(np.float64) * FIX24)[:, None]).astype(np.float32)
    return dict(S=S, cnt=cnt, mean=mean)


def contacts_host(ids, M: int, rows: int, cols: int):
    """(s, t) of every pixel with its right and its lower neighbour where both belong to regions and the regions differ"""
    v = np.asarray(ids, np.int64).reshape(int(rows), int(cols))
    v = np.where((v >= 0) & (v < int(M)), v, -1)
    a = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    b = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    keep = (a >= 0) & (b >= 0) & (a != b)
    return a[keep], b[keep]


def adjacency_host(ids, M: int, rows: int, cols: int, A: int) -> dict:
    """THE DEFINITION OF A REGION ADJACENCY: dict(adj_idx, adj_len int32 [M, A], deg, boundary int32 [M], pairs: the (s, t,
    b[s][t]) of every ordered pair with a contact, sorted by (s, b descending, t ascending))"""
    M, A = int(M), int(A)
    a, b = contacts_host(ids, M, rows, cols)
    s, t = np.concatenate([a, b]), np.concatenate([b, a])
    pair, length = np.unique(s * M + t, return_counts=True)
    ps, pt = pair // M, pair % M
    order = np.lexsort((pt, -length, ps))
    ps, pt, length = ps[order], pt[order], length[order]
    deg = np.bincount(ps, minlength=M)
    boundary = np.bincount(ps, weights=length, minlength=M).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(deg)])[:-1]
    rank = np.arange(len(ps)) - start[ps]
    adj_idx, adj_len = np.full((M, A), -1, np.int32), np.zeros((M, A), np.int32)
    keep = rank < A
    adj_idx[ps[keep], rank[keep]] = pt[keep]
    adj_len[ps[keep], rank[keep]] = length[keep]
    return dict(adj_idx=adj_idx, adj_len=adj_len, deg=deg.astype(np.int32), boundary=boundary.astype(np.int32),
                pairs=(ps, pt, length))


def merge_lists_host(feat, knn_idx, knn_sim, adj_idx):
    """THE DEFINITION OF A REGION GRAPH's lists, with fp64 sims: (nbr_idx int32, nbr_sim float64) [M, k + A]"""
    f = np.asarray(feat, np.float32).astype(np.float64)
    M = f.shape[0]
    knn_idx = np.zeros((M, 0), np.int32) if knn_idx is None else np.asarray(knn_idx, np.int32)
    knn_sim = np.zeros((M, 0), np.float64) if knn_sim is None else np.asarray(knn_sim).astype(np.float64)
    adj = np.zeros((M, 0), np.int32) if adj_idx is None else np.asarray(adj_idx, np.int32)
    k, A = knn_idx.shape[1], adj.shape[1]
    idx, sim = np.full((M, k + A), -1, np.int32), np.full((M, k + A), -np.inf, np.float64)
    idx[:, :k], sim[:, :k] = knn_idx, knn_sim
    for a in range(A):
        t = adj[:, a].astype(np.int64)
        ok = (t >= 0) & (t < M) & ~(knn_idx == adj[:, a:a + 1]).any(1)
        rows = np.nonzero(ok)[0]
        with np.errstate(all="ignore"):
            sim[rows, k + a] = np.einsum("ij,ij->i", f[rows], f[t[rows]])
        idx[rows, k + a] = t[rows]
    return idx, sim


def region_graph_host(ids, M: int, rows: int, cols: int, feat, q, cfg: RegionGraph = RegionGraph(), seeds=None,
                      lists=None, dtype=np.float64) -> dict:
    """The stage on the host from the region descriptors ``feat`` [M, 1024] on: the kNN lists by the definition of the kNN
    vote (leave-one-out), the adjacency, the merged lists (``lists`` = (nbr_idx, nbr_sim): given ones instead, e.g. the
    device's), ``labelprop_host`` from the prior of ``q`` [M, K] (and ``seeds`` = (pix, labels)), and the gather to the pixels.
    dict(nbr_idx, nbr_sim, Y, lp: the LPHost, labels int64 [n], probs [n, K], conf, entropy [n])"""
    from .knn import knn_host
    from .labelprop import labelprop_host
    cfg = RegionGraph(*cfg).check()
    M, k, A = int(M), int(cfg.k), int(cfg.adj)
    ids = np.asarray(ids, np.int64).reshape(-1)
    if lists is None:
        kn = knn_host(feat, feat, None, 0, k, skip=np.arange(M)) if k > 0 else None
        adj = adjacency_host(ids, M, rows, cols, A)
        lists = merge_lists_host(feat, None if kn is None else kn.nbr_idx, None if kn is None else kn.nbr_sim, adj["adj_idx"])
    nbr_idx, nbr_sim = lists
    q = np.asarray(q, np.float32)
    Y = np.where(np.isnan(q), np.float32(0), q)
    inside = (ids >= 0) & (ids < M)
    if seeds is not None:
        from .superpixel import region_vote_host
        tm = np.full(ids.shape[0], -1, np.int64)
        tm[np.asarray(seeds[0], np.int64)] = np.asarray(seeds[1], np.int64)
        vote = region_vote_host(ids, M, q.shape[1], labels=tm)
        Y = np.where((vote["cnt"] > 0)[:, None], vote["q"], Y).astype(np.float32)
    with np.errstate(all="ignore"):
        lp = labelprop_host(nbr_idx, np.asarray(nbr_sim).astype(np.float32), Y, float(cfg.alpha), int(cfg.gamma), int(cfg.iters), dtype=dtype)
    at = np.where(inside, ids, 0)
    nan = np.float64(np.nan)
    return dict(nbr_idx=nbr_idx, nbr_sim=nbr_sim, Y=Y, lp=lp, labels=np.where(inside, lp.labels[at], -1),
                probs=np.where(inside[:, None], lp.probs[at], nan), conf=np.where(inside, lp.conf[at], nan),
                entropy=np.where(inside, lp.entropy[at], nan))
