"""The pseudo-label monitor's host side: the counter block as named fields and rates (``PLCounts``) and the definition
restated in plain numpy (``pl_stats_host`` / ``pl_stats_hard_host``; include/cmlpl.h, "THE DEFINITION OF THE PSEUDO-LABEL
COUNTERS").  The device side is ``cmlpl_pl_stats`` (csrc/plstats.hip), launched by ``TrainEngine(pl_monitor=True)`` behind
every step.  Nothing here touches a GPU."""
from __future__ import annotations

import numpy as np

PL_HEAD = 32
ROW_FIELDS = ("rows", "nan_rows", "sel", "hit_raw", "hit", "sel_hit", "fixed", "broken")     # counts[8 d + s], d = 0, 1
PAIR_FIELDS = ("pairs", "nan_pairs", "pos", "pos_same", "neg", "neg_diff", "launches")       # counts[16 + s]


def pl_size(K: int) -> int:
    """int64 words of the counter block of K classes"""
    return PL_HEAD + 2 * int(K) * int(K)


def _ratio(num, den):
    """num / den elementwise in float64; a zero denominator gives nan, never an exception"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out if out.ndim else float(out)


class PLCounts:
    """The int64 counter block with names.  Per-direction fields (``rows`` .. ``broken``) are int64 arrays [2]: index 0 =
    Base's targets (made by Base1), 1 = Base1's; the graph's (``pairs`` .. ``launches``) are ints; ``cm`` is [2][K][K],
    row = truth, column = pseudo-label, selected rows only.  ``a + b`` adds two blocks (of the same K)."""

    def __init__(self, counts, K: int = None):
        c = np.asarray(counts)
        if c.dtype != np.int64 or c.ndim != 1:
            raise ValueError("PLCounts: a one-dimensional int64 block")
        if K is None:
            K = int(round(((c.size - PL_HEAD) / 2) ** 0.5)) if c.size >= PL_HEAD else -1
        if K < 1 or c.size != pl_size(K):
            raise ValueError(f"PLCounts: {c.size} words is not {PL_HEAD} + 2 K K for a class count K")
        self.K, self.counts = int(K), c.copy()

    @classmethod
    def zeros(cls, K: int) -> "PLCounts":
        return cls(np.zeros(pl_size(K), np.int64), K)

    def __add__(self, other: "PLCounts") -> "PLCounts":
        if not isinstance(other, PLCounts) or other.K != self.K:
            raise ValueError("PLCounts: blocks of the same class count add")
        return PLCounts(self.counts + other.counts, self.K)

    def __eq__(self, other):
        return isinstance(other, PLCounts) and other.K == self.K and bool(np.array_equal(self.counts, other.counts))

    def __getattr__(self, name):
        if name in ROW_FIELDS:
            s = ROW_FIELDS.index(name)
            return self.counts[[s, 8 + s]]
        if name in PAIR_FIELDS:
            return int(self.counts[16 + PAIR_FIELDS.index(name)])
        raise AttributeError(name)

    @property
    def cm(self) -> np.ndarray:
        return self.counts[PL_HEAD:].reshape(2, self.K, self.K)

    # ---- rates: [2] float64 per direction, floats for the graph; nan where nothing was counted
    sel_rate = property(lambda self: _ratio(self.sel, self.rows))                 # share of rows the mask leaves live
    acc_raw = property(lambda self: _ratio(self.hit_raw, self.rows))              # of the plain softmax's label
    acc = property(lambda self: _ratio(self.hit, self.rows))                      # of the (smoothed) target's label
    acc_sel = property(lambda self: _ratio(self.sel_hit, self.sel))               # of the selected rows' labels
    gain = property(lambda self: self.fixed - self.broken)                        # what smoothing changed, in rows
    pos_precision = property(lambda self: _ratio(self.pos_same, self.pos))        # positive edges that join one class
    neg_precision = property(lambda self: _ratio(self.neg_diff, self.neg))        # negative edges that separate two

    @property
    def class_precision(self) -> np.ndarray:
        """[2][K]: of the selected rows given pseudo-label c, the share whose truth is c"""
        cm = self.cm
        return _ratio(np.diagonal(cm, axis1=1, axis2=2), cm.sum(axis=1))

    def __repr__(self):
        return "PLCounts(K=%d, rows=%s, sel=%s, hit=%s, pos=%d, neg=%d, launches=%d)" % (
            self.K, self.rows.tolist(), self.sel.tolist(), self.hit.tolist(), self.pos, self.neg, self.launches)


def _fma32(a, b, c):
    """fl32(a * b + c) of float32 arrays, rounded ONCE (the device's fmaf): the product of two float32 is exact in
    float64; its sum with c is rounded to odd there (the error of the double sum is recovered exactly by two-sum), after
    which the rounding to float32 is the correct rounding of the exact value."""
    x = a.astype(np.float64) * b.astype(np.float64)
    y = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = x + y
        bb = s - x
        err = (x - (s - bb)) + (y - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where((err > 0), np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def graph_q(probs) -> np.ndarray:
    """q[i][j] of the step's pseudo-label graph in its fp32 evaluation: q = 0; for k ascending: q = fmaf(p_s[i][k],
    p_w[j][k], q) -- float32 [btu][btu] (the diagonal as the chain gives it; the step sets its own to 1)"""
    probs = np.asarray(probs, np.float32)
    pw, ps = probs[0], probs[1]
    btu, K = pw.shape
    q = np.zeros((btu, btu), np.float32)
    for k in range(K):
        q = _fma32(np.broadcast_to(ps[:, k:k + 1], (btu, btu)), np.broadcast_to(pw[None, :, k], (btu, btu)), q)
    return q


def _truth_rows(truth, idx, btu):
    truth = np.asarray(truth, np.int64)
    return truth[:btu] if idx is None else truth[np.asarray(idx, np.int64)[:btu]]


def pl_stats_host(probs, truth, idx, adap_mask, pos_thr, neg_thr) -> PLCounts:
    """The definition, restated: ``probs`` float32 [4][btu][K] = p_w, p_s, p_w0, p_s0; ``truth`` int64, read at ``idx[r]``
    (``idx`` None: at r); the three thresholds are compared as float32.  One launch's worth: ``launches`` = 1."""
    probs = np.asarray(probs, np.float32)
    if probs.ndim != 3 or probs.shape[0] != 4:
        raise ValueError("probs: float32 [4][btu][K]")
    _, btu, K = probs.shape
    t = _truth_rows(truth, idx, btu)
    known = (t >= 0) & (t < K)
    adap_mask, pos_thr, neg_thr = np.float32(adap_mask), np.float32(pos_thr), np.float32(neg_thr)
    out = np.zeros(pl_size(K), np.int64)
    cm = out[PL_HEAD:].reshape(2, K, K)
    for d in range(2):
        p, p0 = probs[d], probs[2 + d]
        nan = np.isnan(p).any(axis=1) | np.isnan(p0).any(axis=1)
        ok = known & ~nan
        pz, p0z = np.where(nan[:, None], np.float32(0), p), np.where(nan[:, None], np.float32(0), p0)
        l, l0 = pz.argmax(axis=1), p0z.argmax(axis=1)                 # numpy: the FIRST index of the maximum
        m = ok & (pz[np.arange(btu), l] >= adap_mask)
        hit, hit_raw = ok & (l == t), ok & (l0 == t)
        vals = (known, known & nan, m, hit_raw, hit, m & hit, ok & ~hit_raw & hit, ok & hit_raw & ~hit)
        out[8 * d: 8 * d + 8] = [int(v.sum()) for v in vals]
        np.add.at(cm[d], (t[m], l[m]), 1)
    q = graph_q(probs)
    pair = known[:, None] & known[None, :] & ~np.eye(btu, dtype=bool)
    qnan = np.isnan(q)
    with np.errstate(invalid="ignore"):
        pos, neg = pair & ~qnan & (q >= pos_thr), pair & ~qnan & (q <= neg_thr)
    same = t[:, None] == t[None, :]
    out[16:23] = [int(pair.sum()), int((pair & qnan).sum()), int(pos.sum()), int((pos & same).sum()), int(neg.sum()),
                  int((neg & ~same).sum()), 1]
    return PLCounts(out, K)


def pl_stats_hard_host(pseudo, truth, idx, K: int) -> PLCounts:
    """the definition for hard labels (CPS): ``pseudo`` int64 [2][btu], row 0 = Base's targets"""
    pseudo = np.asarray(pseudo, np.int64)
    if pseudo.ndim != 2 or pseudo.shape[0] != 2:
        raise ValueError("pseudo: int64 [2][btu]")
    btu = pseudo.shape[1]
    t = _truth_rows(truth, idx, btu)
    known = (t >= 0) & (t < K)
    out = np.zeros(pl_size(K), np.int64)
    cm = out[PL_HEAD:].reshape(2, K, K)
    for d in range(2):
        l = pseudo[d]
        bad = known & ((l < 0) | (l >= K))
        sel = known & ~bad
        hit = sel & (l == t)
        out[8 * d: 8 * d + 6] = [int(known.sum()), int(bad.sum()), int(sel.sum()), int(hit.sum()), int(hit.sum()), int(hit.sum())]
        np.add.at(cm[d], (t[sel], l[sel]), 1)
    out[22] = 1
    return PLCounts(out, K)
