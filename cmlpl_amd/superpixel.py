"""Superpixels and region votes, on the device (``cmlpl_sp_segment`` / ``cmlpl_sp_vote_probs`` / ``cmlpl_sp_vote_labels``,
csrc/superpixel.hip; the reference has no counterpart: each of its labels is the product of a single window).

Object-based classification in its three steps: the scene is over-segmented into superpixels -- SLIC (Achanta et al. 2012)
in its per-pixel form (gSLIC, Ren & Reid 2011), on a grid of step S, in the space of the pixel's position and the first
``guide`` channels of the scene cube, its leading z-scored principal components --, every region votes with the class
probabilities (or the labels) of its pixels, and the region is labelled as one.  The definitions, down to the order of the
fp32 operations, are in ``include/cmlpl.h`` ("THE DEFINITION OF A SUPERPIXEL MAP", "THE DEFINITION OF A REGION VOTE");
``segment_host`` and ``region_vote_host`` restate them in numpy, and the tests hold the kernels to those bit for bit.

Not built: moving the seeds to the lowest gradient.  A segment of the plain map need not be connected -- small detached
fragments can exist, confined to a 3 x 3 block of cells; ``Superpixel(connect=True)`` runs SLIC's connectivity post-pass
(cmlpl_amd.regions.connect_segments: the sieve on the segment ids, then the component ids) and votes on that map, every
segment of which is one region.  Nothing else here synchronises; everything runs on the current stream."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .plstats import _fma32

MIN_STEP, MAX_STEP = 2, 64
MAX_ITERS = 100
MAX_GUIDE = 8
MAX_CLASSES = 64
MAX_SEGMENTS = 1 << 24
VOTES = ("soft", "hard")
FIX24 = 16777216.0


def compact_weight(compact: float, step: int) -> np.float32:
    """w = fl32(m^2 / S^2), formed in double from the fp32 m"""
    m = float(np.float32(compact))
    with np.errstate(over="ignore"):
        return np.float32(m * m / (float(step) * float(step)))


class Superpixel(NamedTuple):
    """A grid of ``step`` S pixels (2 .. 64), compactness ``compact`` m (the weight of the distance in the image against the
    distance in the guide), ``iters`` T rounds of assign and update, the first ``guide`` channels of the cube as the guide
    (0: none, a plain grid; clamped to the cube's channels), and the ``vote``: 'soft' sums the class probabilities of a
    region's pixels, 'hard' counts their labels.  ``connect``: the vote runs on the CONNECTED map -- fragments of fewer than
    max(1, S S / 4) pixels join the largest region they touch and every remaining component is a segment of its own
    (``params()`` does not return it: its five values are what the launches of the plain map take).  The defaults are a
    starting point, NOT tuned on any scene."""
    step: int
    compact: float = 1.0
    iters: int = 10
    guide: int = 3
    vote: str = "soft"
    connect: bool = False

    def params(self, channels: Optional[int] = None):
        """(step, compact, iters, guide channels, vote) as the launches take them, checked; ``channels``: the cube's"""
        S, T, G = int(self.step), int(self.iters), int(self.guide)
        if not MIN_STEP <= S <= MAX_STEP:
            raise ValueError(f"Superpixel: step must be {MIN_STEP} .. {MAX_STEP}")
        m = float(self.compact)
        if not (0.0 < m < float("inf")):
            raise ValueError("Superpixel: compact must be finite and > 0")
        w = compact_weight(m, S)
        if not (np.isfinite(w) and w > 0):
            raise ValueError("Superpixel: compact^2 / step^2 must be finite and > 0 in fp32")
        if not 1 <= T <= MAX_ITERS:
            raise ValueError(f"Superpixel: iters must be 1 .. {MAX_ITERS}")
        if not 0 <= G <= MAX_GUIDE:
            raise ValueError(f"Superpixel: guide must be 0 .. {MAX_GUIDE} channels")
        if self.vote not in VOTES:
            raise ValueError("Superpixel: vote must be 'soft' or 'hard'")
        return S, m, T, (G if channels is None else min(G, int(channels))), self.vote


class Segments(NamedTuple):
    seg: torch.Tensor           # int32 [rows * cols]: the segment of every pixel
    centres: torch.Tensor       # float32 [N, 2 + G]: (cy, cx, guide..) after the last update
    counts: torch.Tensor        # int32 [N]: the regular pixels of every segment
    ny: int
    nx: int

    @property
    def N(self) -> int:
        return self.ny * self.nx


class RegionVote(NamedTuple):
    """an ``EnsembleResult`` (``disagree`` None) and, behind it, what the regions said"""
    labels: torch.Tensor                        # int64 [n]; -1: a pixel outside every segment, or of a segment without a vote
    probs: Optional[torch.Tensor] = None        # float32 [n, K]
    conf: Optional[torch.Tensor] = None         # float32 [n]
    entropy: Optional[torch.Tensor] = None      # float32 [n]
    disagree: Optional[torch.Tensor] = None
    seg_probs: Optional[torch.Tensor] = None    # float32 [N, K]: q per segment (NaN: no valid row)
    seg_labels: Optional[torch.Tensor] = None   # int64 [N] (-1: no valid row)
    seg_counts: Optional[torch.Tensor] = None   # int64 [N]: the valid rows of every segment
    sums: Optional[torch.Tensor] = None         # int64 [N, K]: P
    segments: Optional[Segments] = None         # superpixel_probs: the segmenter's map (connect=False: the map that voted)
    connected: Optional[torch.Tensor] = None    # Superpixel(connect=True): int32 [n], the connected map that voted, ids 0 .. M - 1
    M: Optional[int] = None                     # its number of segments


@torch.no_grad()
def segment(cube: torch.Tensor, sp: Superpixel) -> Segments:
    """the superpixel map of the scene ``cube`` [rows, cols, C] (float32 cuda, contiguous) under its first channels"""
    if not (cube.is_cuda and cube.dtype == torch.float32 and cube.dim() == 3 and cube.is_contiguous()):
        raise ValueError("cube: need a contiguous float32 cuda tensor [rows, cols, C]")
    rows, cols, Cc = cube.shape
    S, m, T, G, _ = sp.params(Cc)
    ny, nx = -(-rows // S), -(-cols // S)
    if ny * nx >= MAX_SEGMENTS:
        raise ValueError(f"Superpixel: {ny * nx} segments (the limit is 2^24 - 1)")
    lib, dev = _lib.load(), cube.device
    seg = torch.empty(rows * cols, dtype=torch.int32, device=dev)
    centres = torch.empty(ny * nx, 2 + G, dtype=torch.float32, device=dev)
    counts = torch.empty(ny * nx, dtype=torch.int32, device=dev)
    nbytes = lib.cmlpl_sp_workspace_bytes(rows, cols, G, S)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    _lib.check("cmlpl_sp_segment", lib.cmlpl_sp_segment(
        cube.data_ptr() if G > 0 else None, cube.stride(1), G, rows, cols, S, m, T, seg.data_ptr(), centres.data_ptr(),
        counts.data_ptr(), ws.data_ptr(), nbytes, _lib.stream(dev)))
    return Segments(seg, centres, counts, ny, nx)


@torch.no_grad()
def region_vote(segments, probs: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, K: Optional[int] = None,
                N: Optional[int] = None, probs_out: bool = True, conf: bool = False, entropy: bool = False) -> RegionVote:
    """Every segment of ``segments`` (a ``Segments``, or any int32 cuda map [n] with ``N``) votes: with ``probs`` [n, K]
    (float32, the soft source) or with ``labels`` [n] (int64, the hard source; ``K`` classes).  Per pixel the label of its
    segment and, when asked for, its probabilities / confidence / entropy; per segment always."""
    if isinstance(segments, Segments):
        seg, N = segments.seg, segments.N
    else:
        seg = segments
    if N is None:
        raise ValueError("region_vote: a plain map needs N, the number of segments")
    if (probs is None) == (labels is None):
        raise ValueError("region_vote: one source, probs or labels")
    if not (seg.is_cuda and seg.dtype == torch.int32 and seg.dim() == 1 and seg.is_contiguous()):
        raise ValueError("seg: need a contiguous int32 cuda tensor [n]")
    n, dev = seg.shape[0], seg.device
    if probs is not None:
        if not (probs.is_cuda and probs.dtype == torch.float32 and probs.dim() == 2 and probs.is_contiguous()
                and probs.device == dev and probs.shape[0] == n):
            raise ValueError("probs: need a contiguous float32 cuda tensor [n, K] on the map's device")
        K = probs.shape[1]
    else:
        if not (labels.is_cuda and labels.dtype == torch.int64 and labels.dim() == 1 and labels.is_contiguous()
                and labels.device == dev and labels.shape[0] == n):
            raise ValueError("labels: need a contiguous int64 cuda tensor [n] on the map's device")
        if K is None:
            raise ValueError("region_vote: labels need K, the number of classes")
    N, K = int(N), int(K)
    if not 1 <= K <= MAX_CLASSES or N < 1 or n < 1:
        raise ValueError(f"region_vote: K must be 1 .. {MAX_CLASSES}, N and n at least 1")
    lib = _lib.load()
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    i64 = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
    res = RegionVote(i64(n), f32(n, K) if probs_out else None, f32(n) if conf else None, f32(n) if entropy else None, None,
                     f32(N, K), i64(N), i64(N), i64(N, K))
    nbytes = lib.cmlpl_sp_vote_workspace_bytes(N, K)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    fn, src = ("cmlpl_sp_vote_probs", probs) if probs is not None else ("cmlpl_sp_vote_labels", labels)
    _lib.check(fn, getattr(lib, fn)(
        seg.data_ptr(), src.data_ptr(), n, K, N, _lib.ptr(res.probs), res.labels.data_ptr(), _lib.ptr(res.conf),
        _lib.ptr(res.entropy), res.sums.data_ptr(), res.seg_counts.data_ptr(), res.seg_probs.data_ptr(),
        res.seg_labels.data_ptr(), ws.data_ptr(), nbytes, _lib.stream(dev)))
    return res


@torch.no_grad()
def superpixel_probs(probs: torch.Tensor, cube: torch.Tensor, sp: Superpixel, labels: Optional[torch.Tensor] = None,
                     probs_out: bool = True, conf: bool = False, entropy: bool = False,
                     segments: Optional[Segments] = None) -> RegionVote:
    """``segment(cube, sp)`` (or ``segments``, a map that exists) followed by the vote of ``probs`` [rows * cols, K] over it:
    ``sp.vote`` 'soft' sums the probabilities, 'hard' counts ``labels`` (None: the first maximum of every row of ``probs``).
    The result carries the map as ``.segments``; with ``sp.connect`` the vote runs on ``connect_segments`` of that map (4
    passes, 4-connected, min_size max(1, S S / 4); one word is read back for its M) and the result carries it as ``.connected``."""
    if cube.dim() != 3 or probs.dim() != 2 or probs.shape[0] != cube.shape[0] * cube.shape[1]:
        raise ValueError("probs: need [rows * cols, K] for the cube's scene (a region vote needs the whole map)")
    vote = sp.params(cube.shape[2])[4]
    segs = segment(cube, sp) if segments is None else segments
    voters, extra = (segs,), {}
    if sp.connect:
        from .regions import connect_segments
        S = sp.params()[0]
        ids, M = connect_segments(segs.seg, cube.shape[0], cube.shape[1], max(1, S * S // 4))
        voters, extra = (ids,), dict(N=M)
    if vote == "soft":
        res = region_vote(*voters, probs=probs, probs_out=probs_out, conf=conf, entropy=entropy, **extra)
    else:
        hard = torch.max(probs, 1)[1] if labels is None else labels
        res = region_vote(*voters, labels=hard.contiguous(), K=probs.shape[1], probs_out=probs_out, conf=conf, entropy=entropy,
                          **extra)
    return res._replace(segments=segs, **(dict(connected=voters[0], M=extra["N"]) if sp.connect else {}))


def asa_of_sums(sums) -> float:
    """ASA = sum_s max_c P[s][c] / sum_s cnt[s] of the hard vote of a truth map (NaN: no labelled pixel in any segment)"""
    P = np.asarray(sums.cpu() if torch.is_tensor(sums) else sums, np.int64)
    total = int(P.sum())
    return float(P.max(1).sum()) / total if total > 0 else float("nan")


@torch.no_grad()
def asa(seg, N: int, rows, truth, K: int) -> float:
    """Achievable segmentation accuracy of the map ``seg`` [n] (N segments) on the labelled pixels ``rows`` (indices into
    the map) with classes ``truth``: the best overall accuracy any region-level labelling could reach.  A cuda map is
    hard-voted on the device, a numpy one on the host; the quotient is host arithmetic on P."""
    if torch.is_tensor(seg) and seg.is_cuda:
        on = lambda v: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.int64)))).to(seg.device)
        tm = torch.full((seg.shape[0],), -1, dtype=torch.int64, device=seg.device)
        tm[on(rows).long()] = on(truth).long()
        return asa_of_sums(region_vote(seg, labels=tm, K=K, N=N, probs_out=False).sums)
    seg = np.asarray(seg.cpu() if torch.is_tensor(seg) else seg)
    tm = np.full(seg.shape[0], -1, np.int64)
    tm[np.asarray(rows, np.int64)] = np.asarray(truth, np.int64)
    return asa_of_sums(region_vote_host(seg, N, K, labels=tm)["P"])


# ------------------------------------------------------------------ the definitions, in numpy
def segment_host(cube, step: int, compact: float = 1.0, iters: int = 10, guide: Optional[int] = None) -> dict:
    """THE DEFINITION OF A SUPERPIXEL MAP on ``cube`` [rows, cols, C] (numpy; the first ``guide`` channels, default all):
    dict(seg int32 [n], centres float32 [N, 2 + G], counts int32 [N], ny, nx, changed: pixels relabelled per iteration)"""
    cube = np.asarray(cube, np.float32)
    rows, cols = cube.shape[:2]
    G = cube.shape[2] if guide is None else int(guide)
    S, n = int(step), rows * cols
    g = np.ascontiguousarray(cube[:, :, :G].reshape(n, G))
    w = np.full(n, compact_weight(compact, S), np.float32)
    ny, nx = -(-rows // S), -(-cols // S)
    N = ny * nx
    with np.errstate(invalid="ignore"):
        reg = (np.isfinite(g) & (np.abs(g) <= np.float32(2.0 ** 20))).all(1)
    yy, xx = np.divmod(np.arange(n), cols)
    pa, pb = yy // S, xx // S
    fy, fx = yy.astype(np.float32), xx.astype(np.float32)
    a, b = np.divmod(np.arange(N), nx)
    py, px = np.minimum(rows - 1, a * S + S // 2), np.minimum(cols - 1, b * S + S // 2)
    ci = py * cols + px
    centres = np.zeros((N, 2 + G), np.float32)
    centres[:, 0], centres[:, 1] = py, px
    centres[:, 2:] = np.where(reg[ci, None], g[ci], np.float32(0))
    fix = np.zeros((n, G), np.int64)
    fix[reg] = np.rint(g[reg].astype(np.float64) * FIX24).astype(np.int64)      # llrintf(g * 2^24): the product is exact
    own = (pa * nx + pb).astype(np.int64)
    label, changed = own, []
    for _ in range(int(iters)):
        best, new = np.full(n, np.inf, np.float32), own.copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for da in (-1, 0, 1):
                for db in (-1, 0, 1):
                    ca, cb = pa + da, pb + db
                    ok = reg & (ca >= 0) & (ca < ny) & (cb >= 0) & (cb < nx)
                    s = np.where(ok, ca * nx + cb, 0)
                    c = centres[s]
                    dc2 = np.zeros(n, np.float32)
                    for ch in range(G):
                        d = g[:, ch] - c[:, 2 + ch]
                        dc2 = _fma32(d, d, dc2)
                    dy, dx = fy - c[:, 0], fx - c[:, 1]
                    D = _fma32(_fma32(dx, dx, dy * dy), w, dc2)
                    win = ok & (D < best)
                    best, new = np.where(win, D, best), np.where(win, s, new)
        changed.append(int((new != label).sum()))
        label = new
        lr = label[reg]
        cnt = np.bincount(lr, minlength=N).astype(np.int64)
        Sy, Sx, Sg = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros((N, G), np.int64)
        np.add.at(Sy, lr, yy[reg])
        np.add.at(Sx, lr, xx[reg])
        np.add.at(Sg, lr, fix[reg])
        has = cnt > 0
        dn = cnt[has].astype(np.float64)
        centres[has, 0] = (Sy[has].astype(np.float64) / dn).astype(np.float32)
        centres[has, 1] = (Sx[has].astype(np.float64) / dn).astype(np.float32)
        centres[has, 2:] = (Sg[has].astype(np.float64) / (dn * FIX24)[:, None]).astype(np.float32)
    return dict(seg=label.astype(np.int32), centres=centres, counts=cnt.astype(np.int32), ny=ny, nx=nx, changed=changed)


def region_vote_host(seg, N: int, K: int, probs=None, labels=None) -> dict:
    """THE DEFINITION OF A REGION VOTE: dict(P int64 [N, K], cnt int64 [N], q float32 [N, K], seg_labels int64 [N],
    seg_conf, seg_entropy float32 [N]; labels int64 [n], probs float32 [n, K], conf, entropy float32 [n]).  The entropy
    is the fp32 chain, c ascending, with numpy's logf."""
    seg = np.asarray(seg, np.int64)
    N, K = int(N), int(K)
    inside = (seg >= 0) & (seg < N)
    P = np.zeros((N, K), np.int64)
    if probs is not None:
        p = np.asarray(probs, np.float32)
        with np.errstate(invalid="ignore"):
            valid = inside & (np.isfinite(p) & (p >= 0) & (p <= 2)).all(1)
        np.add.at(P, seg[valid], np.rint(p[valid].astype(np.float64) * FIX24).astype(np.int64))
        scale = FIX24
    else:
        l = np.asarray(labels, np.int64)
        valid = inside & (l >= 0) & (l < K)
        np.add.at(P, (seg[valid], l[valid]), 1)
        scale = 1.0
    cnt = np.bincount(seg[valid], minlength=N).astype(np.int64)
    q = np.full((N, K), np.nan, np.float32)
    has = cnt > 0
    q[has] = (P[has].astype(np.float64) / (cnt[has].astype(np.float64) * scale)[:, None]).astype(np.float32)
    seg_labels = np.full(N, -1, np.int64)
    seg_labels[has] = q[has].argmax(1)                    # (numpy: the first maximum)
    seg_conf = np.full(N, np.nan, np.float32)
    seg_conf[has] = q[has, seg_labels[has]]
    s = np.zeros(N, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(K):
            qc = q[:, c]
            s = s + np.where(qc == 0, np.float32(0), qc * np.log(np.where(qc == 0, np.float32(1), qc)))
    seg_entropy = (np.float32(0) - s).astype(np.float32)
    sc = np.where(inside, seg, 0)
    nan = np.float32(np.nan)
    return dict(P=P, cnt=cnt, q=q, seg_labels=seg_labels, seg_conf=seg_conf, seg_entropy=seg_entropy,
                labels=np.where(inside, seg_labels[sc], -1), probs=np.where(inside[:, None], q[sc], nan),
                conf=np.where(inside, seg_conf[sc], nan), entropy=np.where(inside, seg_entropy[sc], nan))
