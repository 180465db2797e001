"""GPU: ``cmlpl_knn`` / ``cmlpl_embed`` (cmlpl_amd.knn) against include/cmlpl.h, "THE DEFINITION OF A kNN VOTE", as
``cmlpl_amd.knn.knn_host`` / ``vote_host`` restate it in numpy.

The allowance A of a shape is 8 x the largest error of the fp32 ascending chain (the sequential accumulate over d) against
fp64 on the same float32 inputs, computed here for the rows at hand (the convention of tests/test_gpu_ensemble.py): the
kernel's two-piece product is held to what a plain fp32 dot product would be allowed.
  1. every returned similarity is within A of the fp64 similarity of the returned index;
  2. every returned neighbour is a candidate, none repeats, each one's fp64 similarity is >= the k-th fp64 similarity - 2 A,
     and for rows whose fp64 gap between ranks k - 1 and k is >= 4 A the SET is the definition's (at most 10 % left out);
  3. the probabilities against the fp64 vote re-formed from the kernel's OWN list with fp64 similarities: 8 x the fp32
     restatement's own error + 4 A / T (an error A of a similarity moves a weight by A / T relatively; twice for s_r - s_0,
     twice for the ratio);
  4. the labels equal that vote's first maximum where its top-2 gap is >= twice that allowance (at most 5 % left out);
  5. bit for bit: runs, halves, permutations, a query alone; NaN rows, skip, unknown labels, a query without candidates;
  6. embed: bit-equal to the eval forward's feat."""
import functools

import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

D = 1024
SHAPES = [(1, 1, 1, 1), (5, 3, 2, 4), (33, 31, 9, 5), (65, 257, 9, 10), (257, 300, 9, 5), (300, 300, 9, 10),
          (130, 1031, 17, 32), (64, 4097, 64, 1)]
LOO = (300, 300, 9, 10)


def _gen(rng, cent, rows):
    lab = rng.integers(0, cent.shape[0], rows)
    x = np.maximum(cent[lab] + 3.0 * rng.standard_normal((rows, D)), 0.0).astype(np.float32)
    x = (x / np.sqrt((x * x).sum(1, dtype=np.float32))[:, None]).astype(np.float32)
    return x, lab.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(n, m, K, k):
    """(queries, gallery, gallery labels, query truth, skip, fp64 similarities, A) of a shape; shared, never written"""
    rng = np.random.Generator(np.random.PCG64(1000 * n + m + K + k))
    cent = rng.standard_normal((K, D))
    g, lab = _gen(rng, cent, m)
    if (n, m, K, k) == LOO:
        q, truth, skip = g, lab, np.arange(n, dtype=np.int64)
    else:
        (q, truth), skip = _gen(rng, cent, n), None
    S = q.astype(np.float64) @ g.astype(np.float64).T
    chain = np.zeros((n, m), np.float32)
    for d in range(D):                                   # the fp32 ascending chain
        chain = chain + q[:, d:d + 1] * g[None, :, d]
    A = 8.0 * float(np.abs(chain.astype(np.float64) - S).max())
    return q, g, lab, truth, skip, S, A


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(q, g, lab, K, k, T, skip=None):
    from cmlpl_amd.knn import knn
    res = knn(_dev(q), _dev(g), _dev(lab), K, k, T, skip=_dev(skip), neighbours=True)
    return tuple(t.cpu().numpy() for t in res)


def _check(tag, out, q, g, lab, K, k, T, skip, S, A):
    from cmlpl_amd.knn import vote_host
    labels, probs, idx, sim = out
    n, m = S.shape
    ok = np.isfinite(S) & ((lab >= 0) & (lab < K))[None, :]
    if skip is not None:
        ok &= np.arange(m)[None, :] != skip[:, None]
    cand = ok.sum(1)
    have = idx >= 0
    rows = np.arange(n)[:, None]
    safe = np.where(have, idx, 0)
    # the list's shape: min(k, candidates) entries in front, -1 / -inf behind; candidates only, no repeats, in order
    assert np.array_equal(have, np.arange(k)[None, :] < np.minimum(cand, k)[:, None]), tag
    assert np.isneginf(sim[~have]).all() and np.isfinite(sim[have]).all(), tag
    assert ok[rows, safe][have].all(), (tag, "a neighbour that is no candidate")
    srt = np.sort(np.where(have, idx, -1 - np.arange(k)[None, :]), 1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), (tag, "an index repeats")
    both = have[:, 1:]
    assert ((sim[:, :-1] > sim[:, 1:]) | ((sim[:, :-1] == sim[:, 1:]) & (idx[:, :-1] < idx[:, 1:])))[both].all(), (tag, "order")
    # 1. similarities
    s64 = np.where(have, S[rows, safe], -np.inf)
    with np.errstate(invalid="ignore"):
        err = float(np.abs(sim.astype(np.float64) - s64)[have].max()) if have.any() else 0.0
    print(f"[{tag}] A={A:.3e} similarity err={err:.3e}")
    assert err <= A, (tag, err, A)
    # 2. neighbour sets
    Sm = -np.sort(-np.where(ok, S, -np.inf), 1)
    Sm = np.concatenate([Sm, np.full((n, k + 1), -np.inf)], 1)
    kth = Sm[rows[:, 0], np.maximum(np.minimum(cand, k), 1) - 1]
    assert (s64 >= kth[:, None] - 2 * A)[have].all(), (tag, "a neighbour below the k-th similarity")
    with np.errstate(invalid="ignore"):
        gap = Sm[:, k - 1] - Sm[:, k]
    sure = ~(gap < 4 * A)                                  # (fewer than k + 1 candidates: the gap is inf or nan -- nothing to confuse)
    want = np.argsort(np.where(np.where(ok, -S, np.inf) == 0, 0.0, np.where(ok, -S, np.inf)), 1, kind="stable")[:, :k]
    want = np.concatenate([want, np.zeros((n, max(0, k - want.shape[1])), want.dtype)], 1)
    want = np.where(have, want, -1)
    same = (np.sort(want, 1) == np.sort(np.where(have, idx, -1), 1)).all(1)
    left = 1.0 - sure.mean()
    print(f"[{tag}] rows left out of the set equality: {left:.4f}")
    assert same[sure].all(), (tag, "neighbour set", np.nonzero(sure & ~same)[0][:5])
    assert left <= 0.10, (tag, left)
    # 3. probabilities, against the fp64 vote of the kernel's own list
    p64, l64, p32, _ = vote_host(idx, s64, lab, K, T)
    none = ~have[:, 0]
    assert np.isnan(probs[none]).all() and (labels[none] == -1).all(), (tag, "a query without candidates")
    some = ~none
    if some.any():
        own = float(np.abs(p32[some].astype(np.float64) - p64[some]).max())
        tol = 8.0 * own + 4.0 * A / T
        perr = float(np.abs(probs[some].astype(np.float64) - p64[some]).max())
        print(f"[{tag}] restatement err={own:.3e} allowance={tol:.3e} probability err={perr:.3e}")
        assert perr <= tol, (tag, perr, tol)
        # 4. labels
        top = -np.sort(-np.concatenate([p64[some], np.full((int(some.sum()), 1), -np.inf)], 1), 1)
        firm = (top[:, 0] - top[:, 1]) >= 2 * tol
        out_share = 1.0 - firm.mean()
        print(f"[{tag}] rows left out of the label equality: {out_share:.4f}")
        assert np.array_equal(labels[some][firm], l64[some][firm]), (tag, "labels")
        assert out_share <= 0.05, (tag, out_share)


@pytest.mark.parametrize("T", [0.07, 0.3])
@pytest.mark.parametrize("n,m,K,k", SHAPES)
def test_knn_against_the_definition(n, m, K, k, T):
    q, g, lab, truth, skip, S, A = _case(n, m, K, k)
    out = _run(q, g, lab, K, k, T, skip)
    _check(f"{n}x{m} K={K} k={k} T={T}", out, q, g, lab, K, k, T, skip, S, A)
    if skip is not None:
        assert (out[2] != np.arange(n)[:, None]).all()           # leave-one-out: never itself


def test_knn_bit_for_bit():
    n, m, K, k = 257, 300, 9, 5
    q, g, lab, *_ = _case(n, m, K, k)
    T = 0.07
    whole = _run(q, g, lab, K, k, T)
    again = _run(q, g, lab, K, k, T)
    for a, b in zip(whole, again):
        assert np.array_equal(a, b, equal_nan=True), "two runs differ"
    halves = [_run(q[:128], g, lab, K, k, T), _run(q[128:], g, lab, K, k, T)]
    for j, a in enumerate(whole):
        assert np.array_equal(a, np.concatenate([halves[0][j], halves[1][j]]), equal_nan=True), "halves differ from the whole"
    perm = np.random.Generator(np.random.PCG64(3)).permutation(n)
    for a, b in zip(whole, _run(q[perm], g, lab, K, k, T)):
        assert np.array_equal(a[perm], b, equal_nan=True), "a permuted list is not the permuted result"
    for i in (0, 200, 256):
        for a, b in zip(whole, _run(q[i:i + 1], g, lab, K, k, T)):
            assert np.array_equal(a[i:i + 1], b, equal_nan=True), "a query alone differs"
    # the same gallery behind more rows (other tiles, other shares of the gallery): the bits of a similarity stay
    g2 = np.concatenate([g, _case(65, 257, 9, 10)[1]])
    lab2 = np.concatenate([lab, np.full(257, -1, np.int64)])
    for a, b in zip(whole, _run(q, g2, lab2, K, k, T)):
        assert np.array_equal(a, b, equal_nan=True), "masked rows behind the gallery change a result"


def test_knn_nan_rows_skip_and_unknown_labels():
    n, m, K, k = 257, 300, 9, 5
    q, g, lab, _, _, S, A = _case(n, m, K, k)
    q, g, lab, S = q.copy(), g.copy(), lab.copy(), S.copy()
    rng = np.random.Generator(np.random.PCG64(9))
    q[3, 17] = np.nan
    g[5, 100] = np.nan
    S[3, :] = np.nan
    S[:, 5] = np.nan
    lab[rng.integers(0, m, 40)] = -1
    lab[rng.integers(0, m, 40)] = K + 2
    skip = np.where(rng.random(n) < 0.5, S.argsort(1)[:, -2], -1).astype(np.int64)    # half skip a near row (NaN sorts last: [-2] is one)
    for T in (0.07, 0.3):
        out = _run(q, g, lab, K, k, T, skip)
        _check(f"masks T={T}", out, q, g, lab, K, k, T, skip, S, A)
        labels, probs, idx, sim = out
        assert (idx[3] == -1).all() and np.isneginf(sim[3]).all() and np.isnan(probs[3]).all() and labels[3] == -1
        assert (idx != 5).all() and (idx != skip[:, None]).all()
        assert ((lab[idx[idx >= 0]] >= 0) & (lab[idx[idx >= 0]] < K)).all()
    # a query every candidate of which is masked; its neighbour keeps its own
    q2, g2 = q[10:12], g[:3]
    out = _run(q2, g2, np.array([-1, 0, 7]), 2, 4, 0.07, np.array([1, -1]))
    assert out[2].tolist() == [[-1] * 4, [1, -1, -1, -1]] and out[0].tolist() == [-1, 0]
    assert np.isnan(out[1][0]).all() and out[1][1].tolist() == [1.0, 0.0]
    # the search alone: no labels, no vote
    from cmlpl_amd.knn import knn
    res = knn(_dev(q2), _dev(g2), None, 0, 2)
    assert res.labels is None and res.probs is None
    want = (-(q2.astype(np.float64) @ g2.astype(np.float64).T)).argsort(1, kind="stable")[:, :2]
    assert res.nbr_idx.cpu().numpy().tolist() == want.tolist()


def test_knn_refuses_what_it_cannot_take():
    import ctypes as C
    from cmlpl_amd import _lib
    from cmlpl_amd.knn import knn, workspace_bytes
    lib = _lib.load()
    q = torch.zeros(4, D, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    for bad in (dict(k=0), dict(k=33), dict(K=0), dict(K=65), dict(T=0.0)):
        with pytest.raises(ValueError):
            knn(q, q, lab, **{**dict(K=3, k=2, T=0.1), **bad})
    assert lib.cmlpl_knn_workspace_bytes(4, 4, 33) == 0 and lib.cmlpl_knn_workspace_bytes(0, 4, 3) == 0
    ws = torch.empty(workspace_bytes(4, 4, 2), dtype=torch.uint8, device=DEV)
    out = torch.empty(4, dtype=torch.int64, device=DEV)
    call = lambda K, labels, probs, size: lib.cmlpl_knn(q.data_ptr(), 4, q.data_ptr(), 4, labels, K, None, 2, 1.0, None, None,
                                                        probs, out.data_ptr(), ws.data_ptr(), size, None)
    assert call(3, None, None, ws.numel()) == -1                  # K / d_labels without gallery labels
    assert call(3, lab.data_ptr(), None, ws.numel() - 1) == -3
    assert call(3, lab.data_ptr(), None, ws.numel()) == 0
    torch.cuda.synchronize()


def _spe_module(shape, seed, dead=False):
    from cmlpl_amd.models import BaseNet2
    p = O.closed_form_params(shape, seed)
    if dead:                       # non-negative weights, non-positive biases: a spectrum without a positive band is a dead row
        p["feat_spe.weight"] = p["feat_spe.weight"].abs()
        p["feat_spe.bias"] = -p["feat_spe.bias"].abs()
    net = BaseNet2(num_features=shape.bands, dropout=0.8, num_classes=shape.K, in_channels=shape.C, window=shape.H).to(DEV)
    net.load_state_dict(p)
    net.eval()
    return net


@pytest.mark.parametrize("shape", [(103, 11, 11, 103, 9), (200, 11, 11, 200, 16)], ids=["B2", "B4"])
def test_embed_is_the_eval_forwards_feat_bit_for_bit(shape):
    from cmlpl_amd.knn import embed
    s = O.NetShape(*shape)
    rng = np.random.Generator(np.random.PCG64(s.bands))
    nets = (_spe_module(s, 61), _spe_module(s, 62))
    X = torch.from_numpy(rng.standard_normal((300, s.bands)).astype(np.float32)).to(DEV)
    for n in (1, 33, 257):
        rows = torch.from_numpy(rng.integers(0, 300, n).astype(np.int64)).to(DEV)           # scrambled, with repeats at 257
        xs = X[rows].contiguous()
        XP = torch.from_numpy(rng.standard_normal((n, s.C, s.H, s.W)).astype(np.float32)).to(DEV)
        with torch.no_grad():
            want = [net(XP, xs)[1] for net in nets]
        f2, n2 = embed(nets, X, rows)
        assert f2.shape == (2, n, D) and n2.shape == (2, n)
        for j in range(2):
            assert torch.equal(f2[j], want[j]), (shape, n, j, "two networks")
            f1, n1 = embed(nets[j], X, rows)
            assert f1.shape == (n, D) and torch.equal(f1, want[j]) and torch.equal(n1, n2[j]), (shape, n, j, "one network")
            fc, nc = embed(nets[j], xs)                                                       # compact rows, no list
            assert torch.equal(fc, want[j]) and torch.equal(nc, n1)
        assert bool((n2 > 0).all()) and float((f2.double().pow(2).sum(2) - 1).abs().max()) < 1e-5
    assert not torch.equal(f2[0], f2[1])


def test_embed_dead_row():
    from cmlpl_amd.knn import embed
    s = O.NetShape(103, 11, 11, 103, 9)
    net = _spe_module(s, 61, dead=True)
    X = torch.rand(5, s.bands, device=DEV) + 0.5
    X[2] = -X[2]
    feat, norm = embed(net, X)
    assert float(norm[2]) == 0.0 and bool(torch.isnan(feat[2]).all())
    keep = [0, 1, 3, 4]
    assert bool((norm[keep] > 0).all()) and not bool(torch.isnan(feat[keep]).any())
