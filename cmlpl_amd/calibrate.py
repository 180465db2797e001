"""Calibration of the prediction products: does a written confidence mean what it says (include/cmlpl.h, "THE DEFINITION OF
THE RELIABILITY COUNTERS"), and the smallest standard remedy, one scalar temperature (Guo et al., ICML 2017).

``reliability`` counts a probability map against the truth of listed pixels on the device (``cmlpl_reliability``,
csrc/calibrate.hip: integer atomics only, the same bytes on every run) and returns the block as a ``Reliability``: accuracy,
mean confidence, NLL, Brier score, ECE / MCE, the reliability diagram's data and the risk-coverage curve.  ``temper_probs`` is
the map at another temperature, ``q = softmax(log p / T)`` (``cmlpl_temper_probs``); ``fit_temperature`` finds the T of the
least NLL with two launches of ``cmlpl_nll_temps``, 64 candidates each.  ``reliability_host`` / ``temper_host`` /
``nll_temps_host`` restate the definitions in numpy (fp32 chains where the header fixes one): they touch no GPU, and the
tests hold the kernels to them."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

REL_HEAD = 16
HEAD_FIELDS = ("items", "known", "ignored", "nan", "hits", "sum_conf", "sum_nll", "n_inf", "sum_brier")     # counts[s]
FIX24, FIX20 = float(2 ** 24), float(2 ** 20)
BINS_MAX, S_MAX, K_MAX = 1024, 64, 64
BETA_MIN, BETA_MAX = 1.0 / 16.0, 16.0
GRID = 64                                         # candidates per pass of fit_temperature
R1 = 256.0 ** (1.0 / 63.0)                        # ratio of the first pass: 64 values over [1/16, 16]
R2 = R1 ** (2.0 / 63.0)                           # of the second, between the two neighbours of the first minimum: ~1.0028


def rel_size(bins: int) -> int:
    """int64 words of the counter block of ``bins`` bins"""
    return REL_HEAD + 3 * int(bins)


def _ratio(num, den):
    """num / den elementwise in float64; a zero denominator gives nan, never an exception"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out if out.ndim else float(out)


class Reliability:
    """The int64 counter block with names (``items`` .. ``sum_brier``: ints, the sums in units of 2^-24) and what follows
    from it, in float64 on the host.  ``count`` / ``bin_hits`` / ``conf_sum`` are int64 [bins].  ``a + b`` adds two blocks
    (of the same number of bins)."""

    def __init__(self, counts, bins: int = None):
        c = np.asarray(counts)
        if c.dtype != np.int64 or c.ndim != 1:
            raise ValueError("Reliability: a one-dimensional int64 block")
        if bins is None:
            bins = (c.size - REL_HEAD) // 3 if c.size > REL_HEAD else -1
        if bins < 1 or c.size != rel_size(bins):
            raise ValueError(f"Reliability: {c.size} words is not {REL_HEAD} + 3 B for a number of bins B")
        self.bins, self.counts = int(bins), c.copy()

    @classmethod
    def zeros(cls, bins: int) -> "Reliability":
        return cls(np.zeros(rel_size(bins), np.int64), bins)

    def __add__(self, other: "Reliability") -> "Reliability":
        if not isinstance(other, Reliability) or other.bins != self.bins:
            raise ValueError("Reliability: blocks of the same number of bins add")
        return Reliability(self.counts + other.counts, self.bins)

    def __eq__(self, other):
        return isinstance(other, Reliability) and other.bins == self.bins and bool(np.array_equal(self.counts, other.counts))

    def __getattr__(self, name):
        if name in HEAD_FIELDS:
            return int(self.counts[HEAD_FIELDS.index(name)])
        raise AttributeError(name)

    count = property(lambda self: self.counts[REL_HEAD: REL_HEAD + self.bins])
    bin_hits = property(lambda self: self.counts[REL_HEAD + self.bins: REL_HEAD + 2 * self.bins])
    conf_sum = property(lambda self: self.counts[REL_HEAD + 2 * self.bins:])
    scored = property(lambda self: self.known - self.nan)                       # rows that reached a bin

    # ---- what the block says; nan where nothing was counted
    accuracy = property(lambda self: _ratio(self.hits, self.scored))
    mean_conf = property(lambda self: _ratio(self.sum_conf / FIX24, self.scored))
    brier = property(lambda self: _ratio(self.sum_brier / FIX24, self.scored))

    @property
    def nll(self) -> float:
        """mean -log p[t] over the scored rows; inf when a scored row gave its truth no probability"""
        if self.n_inf > 0:
            return float("inf")
        return _ratio(self.sum_nll / FIX24, self.scored)

    def curve(self):
        """the reliability diagram's data: per bin (count int64, accuracy, mean confidence), nan in an empty bin"""
        return self.count.copy(), _ratio(self.bin_hits, self.count), _ratio(self.conf_sum / FIX24, self.count)

    def _gaps(self):
        count, acc, conf = self.curve()
        full = count > 0
        return count[full], np.abs(acc[full] - conf[full])

    @property
    def ece(self) -> float:
        """sum_b count_b / scored * |hits_b / count_b - conf_sum_b / count_b| over the non-empty bins"""
        count, gap = self._gaps()
        return float((count / float(self.scored) * gap).sum()) if count.size else float("nan")

    @property
    def mce(self) -> float:
        count, gap = self._gaps()
        return float(gap.max()) if count.size else float("nan")

    def risk_coverage(self):
        """(coverage, accuracy) from the top bin down, float64 [bins] each: the share of the scored rows whose confidence
        lies in bins b .. B - 1, and the accuracy of those rows (nan while none is covered).  What ``bins = 1024`` is for."""
        n = np.cumsum(self.count[::-1]).astype(np.float64)
        h = np.cumsum(self.bin_hits[::-1]).astype(np.float64)
        return _ratio(n, np.full_like(n, float(self.scored))), _ratio(h, n)

    def line(self, tag: str = "", note: str = "") -> str:
        """the drivers' line"""
        return "Reliability%s: ECE=%.4f MCE=%.4f NLL=%.4f Brier=%.4f conf=%.4f acc=%.4f%s" % (
            tag, self.ece, self.mce, self.nll, self.brier, self.mean_conf, self.accuracy, note)

    def __repr__(self):
        return "Reliability(bins=%d, items=%d, known=%d, nan=%d, hits=%d, n_inf=%d)" % (
            self.bins, self.items, self.known, self.nan, self.hits, self.n_inf)


# ------------------------------------------------------------------ the definitions, restated in numpy
def _items(probs, truth, rows):
    probs = np.asarray(probs, np.float32)
    if probs.ndim != 2 or not 1 <= probs.shape[1] <= K_MAX:
        raise ValueError("probs: float32 [rows][K], K 1 .. 64")
    truth = np.asarray(truth, np.int64).reshape(-1)
    p = probs[:truth.size] if rows is None else probs[np.asarray(rows, np.int64).reshape(-1)]
    if p.shape[0] != truth.size:
        raise ValueError("one row per truth")
    return p, truth


def _first_max(p):
    """the first index of the maximum of every row; a NaN counts as the maximum and the first NaN wins"""
    nan = np.isnan(p)
    return np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, p).argmax(axis=1))


def _group(K: int) -> int:
    return 1 << max(K - 1, 0).bit_length()


def _butterfly(v):
    """sum over the last axis (a power of two wide, padding included) in the order of the kernels' __shfl_xor butterfly, in
    the dtype of ``v``: for o = G / 2 .. 1: v_c = v_c + v_(c xor o); the result is v_0"""
    G = v.shape[-1]
    idx = np.arange(G)
    o = G // 2
    while o > 0:
        v = v + v[..., idx ^ o]
        o //= 2
    return v[..., 0]


def _pad(v, G):
    return np.concatenate([v, np.zeros(v.shape[:-1] + (G - v.shape[-1],), v.dtype)], axis=-1)


def _fix(x, scale):
    """llrintf(x * scale) of float32 values: the product by a power of two is exact, rint rounds ties to even"""
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * scale).astype(np.int64)


def reliability_host(probs, truth, rows=None, bins: int = 15) -> Reliability:
    """The definition: item i scores row ``rows[i]`` of ``probs`` (``rows`` None: row i) against ``truth[i]``."""
    if not 1 <= bins <= BINS_MAX:
        raise ValueError("bins: 1 .. 1024")
    p, t = _items(probs, truth, rows)
    n, K = p.shape
    B = int(bins)
    out = np.zeros(rel_size(B), np.int64)
    known = (t >= 0) & (t < K)
    label = _first_max(p)
    conf = p[np.arange(n), label]
    isnan = known & np.isnan(conf)
    sc = known & ~isnan
    tt = np.where(known, t, 0)
    hit = sc & (label == tt)
    pt = p[np.arange(n), tt]
    with np.errstate(all="ignore"):
        inf = sc & ~(pt > 0)
        x = conf * np.float32(B)                                            # ONE fp32 multiply
        b = np.where(x >= np.float32(B), B - 1, np.where(x > 0, np.trunc(np.where(np.isfinite(x), x, 0)), 0)).astype(np.int64)
        nll = np.float32(0) - np.log(np.where(inf | ~sc, np.float32(1), pt).astype(np.float32))
        d = p - (np.arange(K)[None, :] == tt[:, None]).astype(np.float32)
        brier = _butterfly(_pad((d * d).astype(np.float32), _group(K)))
        fc = _fix(np.where(sc, conf, np.float32(0)), FIX24)
        out[:9] = [n, int(known.sum()), int((~known).sum()), int(isnan.sum()), int(hit.sum()), int(fc[sc].sum()),
                   int(_fix(nll, FIX24)[sc & ~inf].sum()), int(inf.sum()),
                   int(_fix(np.where(sc, brier, np.float32(0)), FIX24)[sc].sum())]
    np.add.at(out, REL_HEAD + b[sc], 1)
    np.add.at(out, REL_HEAD + B + b[hit], 1)
    np.add.at(out, REL_HEAD + 2 * B + b[sc], fc[sc])
    return Reliability(out, B)


def beta_of(T: float) -> float:
    """beta = fl32(1 / T), formed in double"""
    T = float(T)
    if not (T > 0.0 and np.isfinite(T)):
        raise ValueError("temperature: a finite T > 0")
    return float(np.float32(1.0 / T))


def temper_host(probs, T: float):
    """The fp32 chain of cmlpl_temper_probs: (q float32 [n][K], labels int64, conf, entropy float32 [n])."""
    p = np.asarray(probs, np.float32)
    n, K = p.shape
    beta = np.float32(beta_of(T))
    G = _group(K)
    with np.errstate(all="ignore"):
        label = _first_max(p)
        bad = np.isnan(p).any(axis=1) | (p < 0).any(axis=1) | np.isinf(p).any(axis=1) | ~(np.where(np.isnan(p), -np.inf, p).max(axis=1) > 0)
        l = np.log(p).astype(np.float32)
        m = np.where(np.isnan(l), -np.inf, l).max(axis=1, keepdims=True).astype(np.float32)
        e = np.exp((beta * (l - m).astype(np.float32)).astype(np.float32)).astype(np.float32)
        s = _butterfly(_pad(e, G))
        q = (e / s[:, None]).astype(np.float32)
        q[bad] = np.nan
        t = np.where(q == 0, np.float32(0), (q * np.log(q).astype(np.float32)).astype(np.float32)).astype(np.float32)
        ent = (np.float32(0) - _butterfly(_pad(t, G))).astype(np.float32)
    return q, label.astype(np.int64), q[np.arange(n), label], ent


def check_betas(betas):
    b = np.asarray(betas, np.float32).reshape(-1)
    if not 1 <= b.size <= S_MAX:
        raise ValueError("betas: 1 .. 64 candidates")
    if not bool(((b >= np.float32(BETA_MIN)) & (b <= np.float32(BETA_MAX))).all()):
        raise ValueError("betas: every candidate lies in [1/16, 16]")
    return b


def nll_temps_host(probs, truth, rows, betas) -> np.ndarray:
    """The definition of cmlpl_nll_temps, operation for operation: int64 [2][S]."""
    p, t = _items(probs, truth, rows)
    betas = check_betas(betas)
    K = p.shape[1]
    known = (t >= 0) & (t < K)
    p, t = p[known], t[known]
    n = p.shape[0]
    out = np.zeros((2, betas.size), np.int64)
    with np.errstate(all="ignore"):
        pt = p[np.arange(n), t]
        left = ~(pt > 0) | np.isnan(p).any(axis=1) | (p < 0).any(axis=1) | np.isinf(p).any(axis=1)
        out[1, :] = int(left.sum())
        p, t = p[~left], t[~left]
        n = p.shape[0]
        l = np.log(p).astype(np.float32)
        m = l.max(axis=1).astype(np.float32)
        lt = l[np.arange(n), t]
        for s, beta in enumerate(betas):
            z = np.zeros(n, np.float32)
            for c in range(K):                                              # ascending
                z = (z + np.exp((beta * (l[:, c] - m).astype(np.float32)).astype(np.float32)).astype(np.float32)).astype(np.float32)
            nll = (np.log(z).astype(np.float32) - (beta * (lt - m).astype(np.float32)).astype(np.float32)).astype(np.float32)
            out[0, s] = int(_fix(nll, FIX20).sum())
    return out


# ------------------------------------------------------------------ the grid of fit_temperature
def _clip32(b):
    return np.clip(np.asarray(b, np.float64), BETA_MIN, BETA_MAX).astype(np.float32)


def coarse_betas() -> np.ndarray:
    """the first pass: 64 values of beta, log-spaced over [1/16, 16] (ratio 256^(1/63)), float32, ascending"""
    return _clip32(BETA_MIN * R1 ** np.arange(GRID, dtype=np.float64))


def fine_betas(coarse: np.ndarray, j: int) -> np.ndarray:
    """the second pass: 64 values log-spaced between the two neighbours of candidate ``j`` of the first (at an end of the
    grid: between the end and its one neighbour), both ends included, so the bracket holds candidate j"""
    lo, hi = float(coarse[max(j - 1, 0)]), float(coarse[min(j + 1, len(coarse) - 1)])
    b = _clip32(lo * (hi / lo) ** (np.arange(GRID, dtype=np.float64) / (GRID - 1)))
    b[0], b[-1] = np.float32(lo), np.float32(hi)
    return b


def first_min(sums) -> int:
    """the first index of the least sum (exact: the sums are integers)"""
    return int(np.argmin(np.asarray(sums, np.int64)))


def fit_on(nll_temps) -> tuple:
    """the two-pass search on ``nll_temps(betas) -> int64 [2][S]``: (beta float32, its sums column, the 128 candidates).
    NLL is convex in beta (a log-sum-exp minus a linear term), so the minimum over the line lies between the two
    neighbours of the grid's minimum, and the zoom is sound."""
    coarse = coarse_betas()
    s1 = np.asarray(nll_temps(coarse))
    fine = fine_betas(coarse, first_min(s1[0]))
    s2 = np.asarray(nll_temps(fine))
    j = first_min(s2[0])
    return fine[j], s2[:, j], np.concatenate([coarse, fine])


# ------------------------------------------------------------------ the device side
def _check_device_items(probs, truth, rows):
    import torch
    if not (probs.is_cuda and probs.dtype == torch.float32 and probs.dim() == 2 and probs.is_contiguous()):
        raise ValueError("probs: need a contiguous float32 cuda tensor [rows, K]")
    K = probs.shape[1]
    if not 1 <= K <= K_MAX:
        raise ValueError("probs: K 1 .. 64")
    ok = lambda v: v.is_cuda and v.dtype == torch.int64 and v.dim() == 1 and v.is_contiguous() and v.device == probs.device
    if not ok(truth) or (rows is not None and not ok(rows)):
        raise ValueError("truth / rows: contiguous int64 cuda vectors on the device of probs")
    n = truth.shape[0]
    if n < 1 or (rows is None and n > probs.shape[0]) or (rows is not None and rows.shape[0] != n):
        raise ValueError("one truth per listed row (rows None: per leading row of probs), at least one")
    return n, K


def reliability_block(probs, truth, rows=None, bins: int = 15, counts=None):
    """one launch of cmlpl_reliability on the current stream, no synchronisation: the int64 cuda block it ADDED to
    (``counts``, or a fresh zeroed one)"""
    import torch
    from . import _lib
    n, K = _check_device_items(probs, truth, rows)
    if not 1 <= bins <= BINS_MAX:
        raise ValueError("bins: 1 .. 1024")
    if counts is None:
        counts = torch.zeros(rel_size(bins), dtype=torch.int64, device=probs.device)
    elif not (counts.is_cuda and counts.dtype == torch.int64 and counts.shape == (rel_size(bins),) and counts.is_contiguous()):
        raise ValueError("counts: a contiguous int64 cuda block of 16 + 3 bins words")
    _lib.check("cmlpl_reliability", _lib.load().cmlpl_reliability(
        probs.data_ptr(), K, _lib.ptr(rows), truth.data_ptr(), n, int(bins), counts.data_ptr(),
        _lib.stream(probs.device)))
    return counts


def reliability(probs, truth, rows=None, bins: int = 15) -> Reliability:
    """The reliability counters of ``probs`` (float32 cuda [*, K]) against ``truth`` (int64 cuda [n]; item i scores row
    ``rows[i]``, or row i): one launch and one read-back."""
    return Reliability(reliability_block(probs, truth, rows, bins).cpu().numpy(), bins)


def temper_probs(probs, T: float, probs_out: bool = True, conf: bool = False, entropy: bool = False, out=None):
    """``probs`` (float32 cuda [n, K]) at temperature T: an ``EnsembleResult`` of the labels and whatever was asked for.
    ``out``: where the tempered probabilities go (``probs`` itself: in place).  One launch on the current stream, no
    synchronisation -- and none at all at T == 1: the map is returned as it is, with the label, confidence and entropy
    cmlpl_temper_probs gives at beta = 1 only where they are asked for."""
    import torch
    from . import _lib
    from .ensemble import EnsembleResult
    if not (probs.is_cuda and probs.dtype == torch.float32 and probs.dim() == 2 and probs.is_contiguous()):
        raise ValueError("probs: need a contiguous float32 cuda tensor [n, K]")
    n, K = probs.shape
    if n < 1 or not 1 <= K <= K_MAX:
        raise ValueError("probs: at least one row, K 1 .. 64")
    beta = beta_of(T)
    dev = probs.device
    if out is not None and (out.shape != probs.shape or out.dtype != probs.dtype or not out.is_cuda or not out.is_contiguous()):
        raise ValueError("out: a contiguous float32 cuda tensor of the shape of probs")
    if beta == 1.0 and not conf and not entropy:
        # q = p: the host launches nothing for the map; the labels are the first maxima (torch.max's rule is the header's)
        q = probs if out is None or out is probs else out.copy_(probs)
        return EnsembleResult(torch.max(probs, 1)[1], q if probs_out else None)
    q = (out if out is not None else torch.empty_like(probs)) if probs_out or out is not None else None
    res = EnsembleResult(torch.empty(n, dtype=torch.int64, device=dev), q if probs_out else None,
                         torch.empty(n, dtype=torch.float32, device=dev) if conf else None,
                         torch.empty(n, dtype=torch.float32, device=dev) if entropy else None)
    _lib.check("cmlpl_temper_probs", _lib.load().cmlpl_temper_probs(
        probs.data_ptr(), n, K, beta, _lib.ptr(q), _lib.ptr(res.labels), _lib.ptr(res.conf), _lib.ptr(res.entropy),
        _lib.stream(dev)))
    return res


def nll_temps(probs, truth, rows, betas, sums=None):
    """one launch of cmlpl_nll_temps, no synchronisation: the int64 cuda [2][S] it ADDED to"""
    import torch
    from . import _lib
    n, K = _check_device_items(probs, truth, rows)
    b = check_betas(betas)
    if sums is None:
        sums = torch.zeros(2, b.size, dtype=torch.int64, device=probs.device)
    _lib.check("cmlpl_nll_temps", _lib.load().cmlpl_nll_temps(
        probs.data_ptr(), K, _lib.ptr(rows), truth.data_ptr(), n, (C.c_float * b.size)(*b.tolist()),
        int(b.size), sums.data_ptr(), _lib.stream(probs.device)))
    return sums


def fit_temperature(probs, truth, rows: Optional[object] = None):
    """The temperature of the least NLL of ``probs`` against ``truth``: (T, nll_before, nll_after), the mean NLL at T = 1
    (from the reliability counters) and at the fitted T.  TWO launches of cmlpl_nll_temps, 64 candidates each
    (``fit_on``): deterministic, with a resolution of 0.28 % in T."""
    before = reliability(probs, truth, rows, bins=1)
    beta, col, _ = fit_on(lambda betas: nll_temps(probs, truth, rows, betas).cpu().numpy())
    if int(col[1]) > 0 or before.n_inf > 0:
        raise ValueError("fit_temperature: %d of %d pixels give their true class no probability (p_t <= 0 or a row that is no "
                         "probability vector): their NLL is infinite at every temperature" % (max(int(col[1]), before.n_inf), before.known))
    if before.known < 1:
        raise ValueError("fit_temperature: no pixel of known truth")
    return 1.0 / float(beta), before.nll, float(col[0]) / FIX20 / before.known
