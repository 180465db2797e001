"""Connected regions, on the device (``cmlpl_cc_label`` / ``cmlpl_cc_sieve``, csrc/regions.hip; the reference has no
counterpart: nothing in it says which pixels of a map form one region).

``components`` labels the connected components of an int32 map -- the smallest pixel index of every component, its size and
a compact numbering in first-pixel order; ``sieve`` hands every component smaller than ``min_size`` pixels to the largest
large component it touches (the operation GDAL calls sieve, with a parallel merge order), which removes the speckle a
smoothed label map keeps; ``connect_segments`` does both on the ids of a superpixel map, so that every segment of the result
is one region.  The definitions are in ``include/cmlpl.h`` ("THE DEFINITION OF A COMPONENT MAP", "THE DEFINITION OF A SIEVED
MAP"); ``cc_label_host`` and ``sieve_host`` restate them on the host, and the tests hold the kernels to those word for word.

A ``min_size`` near the width of the true regions REMOVES them: on synthetic maps with 7-pixel-wide regions ``min_size`` 16
lowers the accuracy where 4 raises it (tests/test_regions_host.py).  What the sieve buys on a real scene is not measured.

Not built: a sieve inside ``--eval_every`` (a pixel list has no map), GDAL's smallest-first sequential merge order, merging
by class-weighted boundary length, a sharded version, 3-D connectivity.
Nothing here synchronises (``Components.count()`` reads one word back); everything runs on the current stream."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

CONNS = (4, 8)
MAX_PASSES = 16
MAX_MIN_SIZE = (1 << 31) - 1


class Sieve(NamedTuple):
    """Components of fewer than ``min_size`` pixels (1: none) take the label of the largest component of at least
    ``min_size`` pixels that they touch under ``conn`` (4 or 8), ``passes`` times (1 .. 16; a pass that moves nothing ends
    the effect).  NOT tuned on any scene; a ``min_size`` near the size of the true regions removes them."""
    min_size: int
    conn: int = 4
    passes: int = 4

    def params(self):
        """(min_size, conn, passes) as the launches take them, checked"""
        N, c, T = int(self.min_size), int(self.conn), int(self.passes)
        if not 1 <= N <= MAX_MIN_SIZE:
            raise ValueError(f"Sieve: min_size must be 1 .. {MAX_MIN_SIZE}")
        if c not in CONNS:
            raise ValueError("Sieve: conn must be 4 or 8")
        if not 1 <= T <= MAX_PASSES:
            raise ValueError(f"Sieve: passes must be 1 .. {MAX_PASSES}")
        return N, c, T


class Components(NamedTuple):
    comp: torch.Tensor                      # int32 [n]: the smallest pixel index of the pixel's component (-1: void)
    size: Optional[torch.Tensor]            # int32 [n]: the pixels of its component (0: void)
    id: Optional[torch.Tensor]              # int32 [n]: 0 .. M - 1 in the order of the components' first pixels (-1: void)
    M: torch.Tensor                         # int32 [1], on the device

    def count(self) -> int:
        """the number of components (one word read back: this synchronises)"""
        return int(self.M.item())


class SieveResult(NamedTuple):
    labels: torch.Tensor                    # the sieved map, in the dtype it came in (int32 or int64)
    conf: Optional[torch.Tensor]            # float32 [n]: the pixel's own probability of the label it ends with (NaN: none)
    stats: torch.Tensor                     # int32 [passes, 4]: components, small, small with a target, pixels relabelled

    def summary(self) -> dict:
        """the ``sieve:`` line's numbers (one read-back): the first pass's components and small components, the pixels
        relabelled over all passes, the passes that moved a pixel, and the components that are left -- the last pass's count
        when it moved nothing, else None: a merge can join more than two components, so the counters do not say"""
        s = self.stats.cpu().numpy().astype(np.int64)
        return dict(components=int(s[0, 0]), small=int(s[0, 1]), relabelled=int(s[:, 3].sum()),
                    passes_used=int((s[:, 3] > 0).sum()), components_after=int(s[-1, 0]) if s[-1, 3] == 0 else None)


def _map_arg(name, t, rows, cols):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous int32 cuda tensor [rows * cols]")
    rows, cols = int(rows), int(cols)
    if rows < 1 or cols < 1 or rows * cols > MAX_MIN_SIZE or t.shape[0] != rows * cols:
        raise ValueError(f"{name}: need rows, cols >= 1 with rows * cols = {t.shape[0]} pixels (at most 2^31 - 1)")
    return rows, cols


def _workspace(lib, rows, cols, dev):
    nbytes = lib.cmlpl_cc_workspace_bytes(rows, cols)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


@torch.no_grad()
def components(map: torch.Tensor, rows: int, cols: int, conn: int = 4, sizes: bool = False, ids: bool = False) -> Components:
    """the connected components of the int32 cuda ``map`` [rows * cols] (a negative value is void): ``comp`` always, ``size``
    and ``id`` per pixel when asked for, and the device word ``M``"""
    rows, cols = _map_arg("map", map, rows, cols)
    if conn not in CONNS:
        raise ValueError("components: conn must be 4 or 8")
    lib, dev, n = _lib.load(), map.device, rows * cols
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    res = Components(i32(n), i32(n) if sizes else None, i32(n) if ids else None, i32(1))
    ws, nbytes = _workspace(lib, rows, cols, dev)
    _lib.check("cmlpl_cc_label", lib.cmlpl_cc_label(
        map.data_ptr(), rows, cols, int(conn), res.comp.data_ptr(), _lib.ptr(res.size), _lib.ptr(res.id), res.M.data_ptr(),
        ws.data_ptr(), nbytes, _lib.stream(dev)))
    return res


@torch.no_grad()
def sieve(map_or_labels: torch.Tensor, rows: int, cols: int, sv: Sieve, probs: Optional[torch.Tensor] = None) -> SieveResult:
    """the sieved map of ``map_or_labels`` [rows * cols] (int32, or an int64 label tensor, which torch casts to int32 and
    back: the kernels take int32) under ``sv``; with ``probs`` [n, K] (float32) also ``conf``, every pixel's own probability
    of the label it ends with.  The sieve moves labels, never probabilities."""
    min_size, conn, passes = sv.params()
    src = map_or_labels
    if not (torch.is_tensor(src) and src.dtype in (torch.int32, torch.int64)):
        raise ValueError("sieve: need an int32 map or an int64 label tensor")
    v = src.to(torch.int32).contiguous() if src.dtype == torch.int64 else src
    rows, cols = _map_arg("map", v, rows, cols)
    lib, dev, n = _lib.load(), v.device, rows * cols
    K, conf = 0, None
    if probs is not None:
        if not (probs.is_cuda and probs.dtype == torch.float32 and probs.dim() == 2 and probs.is_contiguous()
                and probs.device == dev and probs.shape[0] == n and probs.shape[1] >= 1):
            raise ValueError("probs: need a contiguous float32 cuda tensor [n, K] on the map's device")
        K, conf = probs.shape[1], torch.empty(n, dtype=torch.float32, device=dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.empty(passes, 4, dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(lib, rows, cols, dev)
    _lib.check("cmlpl_cc_sieve", lib.cmlpl_cc_sieve(
        v.data_ptr(), rows, cols, conn, min_size, passes, out.data_ptr(), stats.data_ptr(), _lib.ptr(probs), K,
        _lib.ptr(conf), ws.data_ptr(), nbytes, _lib.stream(dev)))
    return SieveResult(out.to(torch.int64) if src.dtype == torch.int64 else out, conf, stats)


@torch.no_grad()
def connect_segments(seg: torch.Tensor, rows: int, cols: int, min_size: int, conn: int = 4, passes: int = 4):
    """(int32 map of ids 0 .. M - 1, M) from the segment map ``seg``: the sieve on the segment ids -- a detached fragment of
    fewer than ``min_size`` pixels joins the largest large region it touches --, then the component ids of the result, so
    every segment of the output is connected by construction.  M is read back (one word)."""
    res = sieve(seg, rows, cols, Sieve(min_size, conn, passes))
    comps = components(res.labels, rows, cols, conn, ids=True)
    return comps.id, comps.count()


# ------------------------------------------------------------------ the definitions, on the host
def _steps(conn: int):
    if conn not in CONNS:
        raise ValueError("conn must be 4 or 8")
    return ((0, 1), (1, 0)) + (((1, 1), (1, -1)) if conn == 8 else ())


def _pairs(rows: int, cols: int, conn: int):
    """every adjacent pair (i, j), i < j, once: two index arrays"""
    idx = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    a, b = [], []
    for dy, dx in _steps(conn):
        src = idx[:rows - dy, max(0, -dx):cols - max(0, dx)]
        dst = idx[dy:, max(0, dx):cols - max(0, -dx)]
        a.append(src.ravel())
        b.append(dst.ravel())
    return np.concatenate(a), np.concatenate(b)


def cc_label_host(v, rows: int, cols: int, conn: int = 4) -> dict:
    """THE DEFINITION OF A COMPONENT MAP: dict(comp, size, id int32 [n], M int).  A plain union-find over the joined pairs
    (the smaller root wins), so the cost does not depend on how tortuous the components are."""
    v = np.asarray(v, np.int64).reshape(-1)
    rows, cols = int(rows), int(cols)
    n = rows * cols
    if v.shape[0] != n:
        raise ValueError("cc_label_host: the map has not rows * cols pixels")
    a, b = _pairs(rows, cols, conn)
    joined = (v[a] >= 0) & (v[a] == v[b])
    parent = list(range(n))
    for i, j in zip(a[joined].tolist(), b[joined].tolist()):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        while parent[j] != j:
            parent[j] = parent[parent[j]]
            j = parent[j]
        if i < j:
            parent[j] = i
        elif j < i:
            parent[i] = j
    comp = np.empty(n, np.int64)
    for i in range(n):                                  # (parent[i] <= i: the roots in front of i are final)
        comp[i] = comp[parent[i]] if parent[i] != i else i
    void = v < 0
    comp[void] = -1
    roots = comp == np.arange(n)
    size = np.where(void, 0, np.bincount(comp[~void], minlength=n)[np.where(void, 0, comp)])
    rank = np.cumsum(roots) - 1
    ident = np.where(void, -1, rank[np.where(void, 0, comp)])
    return dict(comp=comp.astype(np.int32), size=size.astype(np.int32), id=ident.astype(np.int32), M=int(roots.sum()))


def sieve_host(v, rows: int, cols: int, min_size: int, conn: int = 4, passes: int = 4) -> dict:
    """THE DEFINITION OF A SIEVED MAP: dict(out int32 [n], stats int32 [passes, 4])"""
    u = np.asarray(v, np.int64).reshape(-1).copy()
    rows, cols, min_size = int(rows), int(cols), int(min_size)
    a, b = _pairs(rows, cols, conn)
    a, b = np.concatenate([a, b]), np.concatenate([b, a])           # (both directions)
    stats = np.zeros((int(passes), 4), np.int64)
    for t in range(int(passes)):
        cc = cc_label_host(u, rows, cols, conn)
        comp, size = cc["comp"].astype(np.int64), cc["size"].astype(np.int64)
        ok = (comp[a] >= 0) & (comp[b] >= 0) & (comp[a] != comp[b]) & (size[a] < min_size) & (size[b] >= min_size)
        best = np.zeros(u.shape[0], np.int64)
        np.maximum.at(best, comp[a[ok]], (size[b[ok]] << 32) | (0xFFFFFFFF - comp[b[ok]]))
        roots = np.flatnonzero(comp == np.arange(u.shape[0]))
        small = roots[size[roots] < min_size]
        moved = small[best[small] != 0]
        stats[t] = (len(roots), len(small), len(moved), size[moved].sum())
        key = best[np.where(comp >= 0, comp, 0)]
        move = (comp >= 0) & (size < min_size) & (key != 0)
        target = 0xFFFFFFFF - (key & 0xFFFFFFFF)
        u = np.where(move, u[np.where(move, target, 0)], u)
    return dict(out=u.astype(np.int32), stats=stats.astype(np.int32))


def connect_segments_host(seg, rows: int, cols: int, min_size: int, conn: int = 4, passes: int = 4):
    """``connect_segments`` on the host: (int32 ids [n], M)"""
    cc = cc_label_host(sieve_host(seg, rows, cols, min_size, conn, passes)["out"], rows, cols, conn)
    return cc["id"], cc["M"]
