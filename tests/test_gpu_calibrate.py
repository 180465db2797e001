"""GPU: the calibration kernels (cmlpl_reliability, cmlpl_temper_probs, cmlpl_nll_temps; csrc/calibrate.hip) against their
definitions in numpy (cmlpl_amd.calibrate, held to hand-made blocks and scalar restatements by tests/test_calibrate_host.py).

Every COUNT of the reliability block, and every sum of confidences (a value read, never computed: llrintf(conf 2^24) is
exact on both sides), is an equality of integers.  The decisions behind them are comparisons of values the kernel reads;
only the first maximum could be decided otherwise by another evaluation, so the random fixtures keep the top-2 gap of every
row >= 1e-3 -- rows are drawn again until it holds (at most 8 rounds), the margin is asserted, nothing is left out.
Where the device's expf / logf enter (sum_nll, sum_brier's order, the tempered probabilities, the NLL sums) the kernels are
held to the fp64 definition with 8 x the error the fp32 numpy restatement itself has against fp64 -- the convention of
tests/test_gpu_ensemble.py -- plus half a unit per row where a value is rounded to fixed point."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmlpl_amd import calibrate as cal
from cmlpl_amd.calibrate import FIX20, FIX24, REL_HEAD, Reliability, nll_temps_host, reliability_host, rel_size, temper_host
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
GAP = 1e-3
NAN = float("nan")
# no full group; a wave boundary; K across the group widths; more than one workgroup with a tail
SHAPES = ((1, 1), (5, 2), (63, 9), (64, 9), (65, 9), (1000, 16), (1031, 17), (4097, 64))
BINS = (1, 2, 15, 64, 1024)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _lib():
    from cmlpl_amd import _lib
    return _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _softmax64(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _gap(p):
    if p.shape[1] < 2:
        return np.full(p.shape[0], np.inf)
    top = np.sort(p.astype(np.float64), axis=1)
    return top[:, -1] - top[:, -2]


def make_probs(rows, K, seed, scale=2.0):
    """float32 softmax rows whose top-2 gap is >= GAP (asserted); returns (probs, redraw rounds)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    draw = lambda m: _softmax64(scale * rng.standard_normal((m, K))).astype(np.float32)
    p, rounds = draw(rows), 0
    while True:
        bad = _gap(p) < GAP
        if not bad.any():
            break
        rounds += 1
        assert rounds <= 8, "the fixture does not converge"
        p[bad] = draw(int(bad.sum()))
    assert (_gap(p) >= GAP).all()
    return p, rounds


def make_truth(p, seed, unknown=True):
    rng = np.random.Generator(np.random.PCG64(seed + 77))
    n, K = p.shape
    t = p.argmax(axis=1).astype(np.int64)
    wrong = rng.random(n) < 0.3
    t[wrong] = rng.integers(0, K, int(wrong.sum()))
    if unknown and n >= 5:                                # truths out of range, on both sides
        out = rng.choice(n, max(2, n // 16), replace=False)
        t[out[::2]], t[out[1::2]] = -1, K
    return t


def _differing(got, want):
    bad = np.nonzero(got != want)[0]
    return [(int(i), int(got[i]), int(want[i])) for i in bad[:12]]


def _rel(probs, truth, rows, bins, counts=None):
    blk = cal.reliability_block(_dev(probs), _dev(truth), None if rows is None else _dev(rows), bins, counts)
    torch.cuda.synchronize()
    return blk


EXACT_HEAD = (0, 1, 2, 3, 4, 5, 7)                        # items known ignored nan hits sum_conf n_inf


def _check_block(got, probs, truth, rows, bins, tag):
    """every integer word equal to the definition's; sum_nll and sum_brier inside their allowance of the fp64 definition"""
    want = reliability_host(probs, truth, rows, bins)
    exact = np.ones(rel_size(bins), bool)
    exact[[6, 8]] = False
    assert not _differing(got[exact], want.counts[exact]), (tag, _differing(got[exact], want.counts[exact]))
    assert not got[9:REL_HEAD].any()
    # the two computed sums, against fp64 on the float32 values the kernel reads
    p = (probs if rows is None else probs[rows])[:len(truth)]
    K = p.shape[1]
    known = (truth >= 0) & (truth < K)
    sc = known & ~np.isnan(p).any(axis=1)
    tt = np.where(known, truth, 0)
    p64 = p.astype(np.float64)
    with np.errstate(all="ignore"):
        pt = p64[np.arange(len(p)), tt]
        fin = sc & (pt > 0)
        nll64 = -np.log(np.where(fin, pt, 1.0))
        nll32 = (np.float32(0) - np.log(np.where(fin, pt, 1.0).astype(np.float32))).astype(np.float64)
        onehot = np.arange(K)[None, :] == tt[:, None]
        brier64 = ((p64 - onehot) ** 2).sum(axis=1)
        d = p - onehot.astype(np.float32)
        brier32 = cal._butterfly(cal._pad((d * d).astype(np.float32), cal._group(K))).astype(np.float64)
    for word, name, v64, v32, on in ((6, "sum_nll", nll64, nll32, fin), (8, "sum_brier", brier64, brier32, sc)):
        ref = float(v64[on].sum()) * FIX24
        allow = 8 * float(np.abs(v32[on] - v64[on]).sum()) * FIX24 + 0.5 * int(on.sum())
        print("%s %s: device %d host %d fp64 %.1f allowed %.1f" % (tag, name, got[word], want.counts[word], ref, allow))
        assert abs(int(got[word]) - ref) <= allow, (tag, name, int(got[word]), ref, allow)
    return want


# ------------------------------------------------------------------ cmlpl_reliability
@pytest.mark.parametrize("n,K", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_reliability_equals_the_definition_word_for_word(n, K):
    probs, rounds = make_probs(n, K, 100 * n + K)
    truth = make_truth(probs, n)
    # the same items through a list with duplicates, in descending order, over a larger map
    big, _ = make_probs(n + 37, K, 100 * n + K + 1)
    rng = np.random.Generator(np.random.PCG64(n))
    rows = np.sort(rng.integers(0, n + 37, n))[::-1].astype(np.int64).copy()
    if n > 2:
        rows[1] = rows[0]
    truth_big = make_truth(big[rows], n + 1)
    for bins in BINS:
        want = _check_block(_rel(probs, truth, None, bins).cpu().numpy(), probs, truth, None, bins, "%dx%d B%d" % (n, K, bins))
        _check_block(_rel(big, truth_big, rows, bins).cpu().numpy(), big, truth_big, rows, bins, "%dx%d B%d list" % (n, K, bins))
    print("n %d K %d: redraw rounds %d; %r" % (n, K, rounds, want))
    assert want.items == n and want.known + want.ignored == n and (want.hits > 0 or n == 1)
    if n >= 63:
        assert want.ignored >= 2 and 0 < want.hits < want.scored and (K == 1 or np.count_nonzero(want.count) > 1)


def test_reliability_nan_rows_ties_edges_and_the_hand_block():
    from tests.test_calibrate_host import hand_block
    probs, truth = hand_block()
    got = _rel(probs, truth, None, 4).cpu().numpy()
    want = _check_block(got, probs, truth, None, 4, "hand block")
    assert want.sum_brier == got[8]                       # every value dyadic: only sum_nll's logf of 0.5 and 0.625 is computed
    assert Reliability(got, 4).nll == float("inf") and Reliability(got, 4).ece == 0.40625
    # NaN rows among random ones, conf > 1 and < 0, K = 9
    p, _ = make_probs(300, 9, 5)
    t = make_truth(p, 5)
    p[::17, 3] = NAN
    p[5] = NAN
    p[6] = [1.5, 0, 0, 0, 0, 0, 0, 0, 0]
    p[7] = [-0.5, -1, -1, -1, -1, -1, -1, -1, -1]
    t[5:8] = 0
    for bins in (8, 15):
        w = _check_block(_rel(p, t, None, bins).cpu().numpy(), p, t, None, bins, "nan B%d" % bins)
        nan_known = int((np.isnan(p).any(axis=1) & (t >= 0) & (t < 9)).sum())      # (a NaN row of unknown truth is `ignored`)
        assert w.nan == nan_known >= 10 and w.n_inf >= 1


def test_reliability_every_row_in_one_bin():
    """LDS-atomic contention: 4097 scored rows, one cell"""
    n, K = 4097, 9
    p = np.full((n, K), 0.01, np.float32)
    p[:, 4] = 0.92
    t = np.full(n, 4, np.int64)
    t[::3] = 2
    for bins in (15, 1024):
        got = _rel(p, t, None, bins).cpu().numpy()
        want = _check_block(got, p, t, None, bins, "one bin B%d" % bins)
        assert np.count_nonzero(want.count) == 1 and want.count.max() == n and want.hits == n - len(t[::3])


def test_reliability_launches_add_up_bit_for_bit():
    p, _ = make_probs(1031, 17, 9)
    t = make_truth(p, 9)
    whole = _rel(p, t, None, 64)
    rows = np.arange(1031, dtype=np.int64)
    halves = _rel(p, t[:500], None, 64)
    halves = _rel(p, t[500:], rows[500:], 64, counts=halves)
    assert torch.equal(whole, halves)
    assert torch.equal(_rel(p, t, None, 64), whole)                             # the same bytes on every run
    twice = _rel(p, t, None, 64, counts=whole.clone())
    assert torch.equal(twice, 2 * whole)
    r = cal.reliability(_dev(p), _dev(t), None, 64)
    assert r == Reliability(whole.cpu().numpy()) and r.items == 1031


def test_arguments_are_checked():
    lib, E_ARG = _lib(), -1
    f = torch.full((64,), 0.5, dtype=torch.float32, device=DEV)
    d = torch.zeros(64, dtype=torch.int64, device=DEV)
    blk = torch.zeros(rel_size(4), dtype=torch.int64, device=DEV)
    st = _stream()
    rel = lib.cmlpl_reliability
    assert rel(None, 2, None, d.data_ptr(), 4, 4, blk.data_ptr(), st) == E_ARG
    assert rel(f.data_ptr(), 2, None, None, 4, 4, blk.data_ptr(), st) == E_ARG
    assert rel(f.data_ptr(), 2, None, d.data_ptr(), 4, 4, None, st) == E_ARG
    assert rel(f.data_ptr(), 0, None, d.data_ptr(), 4, 4, blk.data_ptr(), st) == E_ARG
    assert rel(f.data_ptr(), 65, None, d.data_ptr(), 1, 4, blk.data_ptr(), st) == E_ARG
    assert rel(f.data_ptr(), 2, None, d.data_ptr(), 0, 4, blk.data_ptr(), st) == E_ARG
    assert rel(f.data_ptr(), 2, None, d.data_ptr(), 4, 0, blk.data_ptr(), st) == E_ARG
    assert rel(f.data_ptr(), 2, None, d.data_ptr(), 4, 1025, blk.data_ptr(), st) == E_ARG
    assert rel(f.data_ptr(), 2, None, d.data_ptr(), 4, 4, blk.data_ptr() + 4, st) == E_ARG
    tmp = lib.cmlpl_temper_probs
    for beta in (0.0, -1.0, float("inf"), NAN):
        assert tmp(f.data_ptr(), 4, 2, beta, f.data_ptr(), None, None, None, st) == E_ARG
    assert tmp(None, 4, 2, 1.0, None, None, None, None, st) == E_ARG
    assert tmp(f.data_ptr(), 0, 2, 1.0, None, None, None, None, st) == E_ARG
    assert tmp(f.data_ptr(), 1, 65, 1.0, None, None, None, None, st) == E_ARG
    nll = lib.cmlpl_nll_temps
    sums = torch.zeros(2, 64, dtype=torch.int64, device=DEV)
    b = lambda *v: (C.c_float * len(v))(*v)
    assert nll(f.data_ptr(), 2, None, d.data_ptr(), 4, b(1.0), 0, sums.data_ptr(), st) == E_ARG
    assert nll(f.data_ptr(), 2, None, d.data_ptr(), 4, b(*[1.0] * 65), 65, sums.data_ptr(), st) == E_ARG
    assert nll(f.data_ptr(), 2, None, d.data_ptr(), 4, None, 1, sums.data_ptr(), st) == E_ARG
    for bad in (0.06, 16.5, NAN, -1.0):
        assert nll(f.data_ptr(), 2, None, d.data_ptr(), 4, b(1.0, bad), 2, sums.data_ptr(), st) == E_ARG
    assert nll(f.data_ptr(), 2, None, d.data_ptr(), 0, b(1.0), 1, sums.data_ptr(), st) == E_ARG
    torch.cuda.synchronize()
    assert not blk.any() and not sums.any() and bool((f == 0.5).all())


# ------------------------------------------------------------------ cmlpl_temper_probs
TEMPS = (1 / 16, 0.5, 1.0, 2.03, 16.0)


def _temper(p, T, **kw):
    res = cal.temper_probs(_dev(p), T, probs_out=True, conf=True, entropy=True, **kw)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("K", [1, 2, 3, 5, 9, 16, 17, 64])            # every lane group: G = 1, 2, 4, 8, 16, 16, 32, 64
def test_temper_probs_against_the_fp64_definition(K):
    n = 517                                               # more than one workgroup at every K, with a tail
    p, _ = make_probs(n, K, 40 + K)
    p64 = p.astype(np.float64)
    for T in TEMPS:
        beta = float(np.float32(1.0 / T))
        with np.errstate(divide="ignore"):
            q64 = _softmax64(beta * np.log(p64))
        with np.errstate(divide="ignore", invalid="ignore"):
            e64 = -np.where(q64 > 0, q64 * np.log(np.where(q64 > 0, q64, 1.0)), 0.0).sum(axis=1)
        qh, lh, ch, eh = temper_host(p, T)
        res = _temper(p, T)
        lab, q, conf, ent = (v.cpu().numpy() for v in res[:4])
        tol_q, tol_e = 8 * np.abs(qh - q64).max(), 8 * np.abs(eh - e64).max()
        err_q, err_e = np.abs(q - q64).max(), np.abs(ent - e64).max()
        print("K %d T %g: q err %.2e (allowed %.2e) entropy err %.2e (allowed %.2e)" % (K, T, err_q, tol_q, err_e, tol_e))
        assert err_q <= tol_q and err_e <= tol_e
        assert np.array_equal(lab, p.argmax(axis=1)) and np.array_equal(lab, lh)
        assert np.array_equal(conf, q[np.arange(n), lab]) and np.array_equal(conf, q.max(axis=1))
        assert np.abs(q.astype(np.float64).sum(axis=1) - 1).max() <= 2 * K * 2.0 ** -24


def test_temper_probs_special_rows_bit_for_bit():
    p = np.array([[0.5, 0.5, 0.0], [NAN, 0.5, 0.5], [0.0, 0.0, 0.0], [0.5, -0.1, 0.6], [0.25, 0.0, 0.75], [0.3, 0.3, 0.4],
                  [0.2, NAN, NAN], [0.0, 1.0, 0.0], [np.inf, 0.5, 0.5]], np.float32)
    for T in (0.5, 2.0, 16.0):
        qh, lh, ch, eh = temper_host(p, T)
        lab, q, conf, ent = (v.cpu().numpy() for v in _temper(p, T)[:4])
        assert lab.tolist() == lh.tolist() == [0, 0, 0, 2, 2, 2, 1, 1, 0]
        assert np.array_equal(np.isnan(q), np.isnan(qh)) and np.isnan(q[[1, 2, 3, 6, 8]]).all() and not np.isnan(q[[0, 4, 5, 7]]).any()
        assert np.array_equal(np.isnan(conf), np.isnan(ch)) and np.array_equal(np.isnan(ent), np.isnan(eh))
        assert q[0].tobytes() == np.array([0.5, 0.5, 0.0], np.float32).tobytes()          # a tie stays a tie, the zero exact
        assert q[7].tobytes() == np.array([0.0, 1.0, 0.0], np.float32).tobytes() and ent[7] == 0.0
        assert q[4, 1] == 0.0 and q[5, 0] == q[5, 1] and conf[0] == 0.5 and conf[7] == 1.0
    # any output may be left out
    d = _dev(p)
    only = cal.temper_probs(d, 2.0, probs_out=False, conf=True)
    assert only.probs is None and only.entropy is None and torch.equal(only.labels.cpu(), torch.tensor([0, 0, 0, 2, 2, 2, 1, 1, 0]))


def test_temper_probs_in_place_position_and_repeat():
    p, _ = make_probs(1031, 9, 8)
    a = _temper(p, 2.03)
    b = _temper(p, 2.03)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)                          # the same bytes on two runs
    d = _dev(p)
    c = cal.temper_probs(d, 2.03, probs_out=True, conf=True, entropy=True, out=d)          # in place
    torch.cuda.synchronize()
    assert c.probs.data_ptr() == d.data_ptr()
    for x, y in zip(a[:4], c[:4]):
        assert torch.equal(x, y)
    # a row's bytes do not depend on where in the launch it lies
    shifted = np.concatenate([p[-5:], p])
    s = _temper(shifted, 2.03)
    for x, y in zip(a[:4], s[:4]):
        assert torch.equal(x, y[5:])
    # T == 1: the map as it is, no launch asked of the library
    one = cal.temper_probs(_dev(p), 1.0)
    assert torch.equal(one.probs.cpu(), torch.from_numpy(p)) and np.array_equal(one.labels.cpu().numpy(), p.argmax(axis=1))


# ------------------------------------------------------------------ cmlpl_nll_temps
def _betas(S):
    return cal.coarse_betas()[np.round(np.linspace(0, 63, S)).astype(int)] if S > 1 else np.array([0.4926], np.float32)


@pytest.mark.parametrize("n,K", [(1, 2), (65, 9), (4096, 9), (1031, 64)], ids=["1x2", "65x9", "4096x9", "1031x64"])
def test_nll_temps_against_the_definition(n, K):
    p, _ = make_probs(n + 11, K, 300 + n)
    rng = np.random.Generator(np.random.PCG64(n))
    rows = rng.permutation(n + 11)[:n].astype(np.int64)
    truth = make_truth(p[rows], n)
    if n >= 65:                                            # rows that are left out: p_t = 0, a NaN beside the truth
        k = [i for i in range(n) if 0 <= truth[i] < K][:2]
        p[rows[k[0]], truth[k[0]]] = 0.0
        p[rows[k[1]], (truth[k[1]] + 1) % K] = NAN
    dp, dr, dt = _dev(p), _dev(rows), _dev(truth)
    for S in (1, 33, 64):
        betas = _betas(S)
        want = nll_temps_host(p, truth, rows, betas)
        got = cal.nll_temps(dp, dt, dr, betas)
        torch.cuda.synchronize()
        g = got.cpu().numpy()
        diff = np.abs(g[0] - want[0])
        print("n %d K %d S %d: max |device - host| = %d units of 2^-20 (allowed %d); left out %d; mean nll %.4f .. %.4f" %
              (n, K, S, diff.max(), n, want[1, 0], g[0].min() / FIX20 / n, g[0].max() / FIX20 / n))
        assert g.shape == (2, S) and np.array_equal(g[1], want[1]) and (want[1] == (2 if n >= 65 else 0)).all()
        assert diff.max() <= n
        # chunked == whole, bit for bit; and the same bytes again
        h = n // 2
        parts = cal.nll_temps(dp, dt[:h].contiguous(), dr[:h].contiguous(), betas) if h else torch.zeros_like(got)
        parts = cal.nll_temps(dp, dt[h:].contiguous(), dr[h:].contiguous(), betas, sums=parts)
        assert torch.equal(parts, got) and torch.equal(cal.nll_temps(dp, dt, dr, betas), got)
    # rows None: the leading rows
    got = cal.nll_temps(dp, _dev(make_truth(p[:n], 3)), None, _betas(33)).cpu().numpy()
    assert np.abs(got[0] - nll_temps_host(p, make_truth(p[:n], 3), None, _betas(33))[0]).max() <= n


# ------------------------------------------------------------------ fit_temperature
def _golden(f, lo, hi, iters=80):
    g = (np.sqrt(5.0) - 1) / 2
    a, b = lo, hi
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(iters):
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = f(d)
    return (a + b) / 2


def test_fit_temperature_finds_the_fp64_optimum_and_lowers_ece():
    """logits over-confident by a factor 2: labels drawn from softmax(z0), probabilities softmax(2 z0); n = 4096 fits, a
    disjoint 4096 scores"""
    rng = np.random.Generator(np.random.PCG64(1088))
    n, K = 4096, 9
    z0 = rng.standard_normal((2 * n, K))
    true = _softmax64(z0)
    labels = (true.cumsum(axis=1) < rng.random((2 * n, 1))).sum(axis=1).clip(0, K - 1).astype(np.int64)
    p = _softmax64(2 * z0).astype(np.float32)
    dp, dt = _dev(p), _dev(labels)
    fit_rows, held_rows = torch.arange(n, device=DEV), torch.arange(n, 2 * n, device=DEV)
    T, before, after = cal.fit_temperature(dp, dt[:n].contiguous(), fit_rows)
    logp = np.log(p[:n].astype(np.float64))

    def nll64(logT):
        s = logp / np.exp(logT)
        return float((np.log(np.exp(s - s.max(axis=1, keepdims=True)).sum(axis=1)) + s.max(axis=1) - s[np.arange(n), labels[:n]]).mean())
    T64 = float(np.exp(_golden(nll64, np.log(1 / 16), np.log(16.0))))
    print("fitted T %.5f, fp64 optimum %.5f, ratio %.6f (allowed %.6f); NLL %.4f -> %.4f" %
          (T, T64, max(T / T64, T64 / T), cal.R2 ** 2, before, after))
    assert max(T / T64, T64 / T) <= cal.R2 ** 2
    assert abs(before - nll64(0.0)) < 1e-4 and abs(after - nll64(np.log(T))) < 1e-4 and after < before
    again = cal.fit_temperature(dp, dt[:n].contiguous(), fit_rows)
    assert again == (T, before, after)
    raw = cal.reliability(dp, dt[n:].contiguous(), held_rows)
    tempered = cal.reliability(cal.temper_probs(dp, T).probs, dt[n:].contiguous(), held_rows)
    print("held-out ECE %.4f -> %.4f, NLL %.4f -> %.4f" % (raw.ece, tempered.ece, raw.nll, tempered.nll))
    assert tempered.ece < raw.ece and tempered.nll < raw.nll and tempered.hits == raw.hits
    # a pixel whose true class has no probability: refused with the reason
    bad = p[:n].copy()
    bad[3, labels[3]] = 0.0
    with pytest.raises(ValueError, match="no probability"):
        cal.fit_temperature(_dev(bad), dt[:n].contiguous())
