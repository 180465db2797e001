"""What the label-propagation tests share: the arcs (nine neighbouring meridian arcs of one sphere, embedded in 1024-D), the
random hub graphs, and the comparison of a device result with the host's definition."""
import functools

import numpy as np

ARC_CASES = ((60, 0.35, 6), (120, 0.30, 8))          # (n_per, the angle between neighbouring arcs, k)
ARC_ALPHA, ARC_GAMMA, ARC_ITERS = 0.99, 3, 100


@functools.lru_cache(maxsize=None)
def arcs(n_per, dphi, classes=9):
    """(X float32 [9 n_per, 1024] unit rows, truth int64, seed_labels int64 (-1 = no seed)), drawn in the order written:
    Q, then per class the angles t and the noise (PCG64 seed 1); five seeds per class (PCG64 seed 2)"""
    rng = np.random.Generator(np.random.PCG64(1))
    Q, _ = np.linalg.qr(rng.standard_normal((1024, 3)))
    rows, truth = [], []
    for c in range(classes):
        t = rng.uniform(0.35, 2.8, n_per)
        phi = c * dphi
        p = np.stack([np.cos(t), np.sin(t) * np.cos(phi), np.sin(t) * np.sin(phi)], 1) + 0.01 * rng.standard_normal((n_per, 3))
        x = p @ Q.T
        rows.append(x / np.linalg.norm(x, axis=1, keepdims=True))
        truth.append(np.full(n_per, c, np.int64))
    X, truth = np.concatenate(rows), np.concatenate(truth)
    rng2 = np.random.Generator(np.random.PCG64(2))
    seeds = np.full(len(truth), -1, np.int64)
    for c in range(classes):
        pick = c * n_per + rng2.choice(n_per, 5, replace=False)
        seeds[pick] = c
    X.setflags(write=False), truth.setflags(write=False), seeds.setflags(write=False)
    return X.astype(np.float32), truth, seeds


def exact_neighbours(X, k):
    """(idx int32 [n, k], sim float64 [n, k]) by exact fp64 cosine, self excluded, (s descending, j ascending)"""
    x = np.asarray(X, np.float64)
    S = x @ x.T
    np.fill_diagonal(S, -np.inf)
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(S, order, 1)


def nearest_seed_accuracy(X, truth, seeds):
    x = np.asarray(X, np.float64)
    at = np.nonzero(seeds >= 0)[0]
    return float((seeds[at][(x @ x[at].T).argmax(1)] == truth).mean())


def one_hot(labels, K, dtype=np.float32):
    Y = np.zeros((len(labels), K), dtype)
    ok = (labels >= 0) & (labels < K)
    Y[np.nonzero(ok)[0], labels[ok]] = 1
    return Y


@functools.lru_cache(maxsize=None)
def hub_graph(n, k, K, seed=0, dense=False):
    """random lists with node 0 forced into every other row: (idx int32 [n, k], sim float32 [n, k], Y float32 [n, K]).
    Similarities U(-0.2, 1), descending per row; a tenth of the rows truncated by pads; max(3 K, 20) random seeds (or a
    dense random non-negative Y)"""
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    idx = np.empty((n, k), np.int32)
    for i in range(n):                                   # (the hub at a random rank)
        others = np.delete(np.arange(1, n), i - 1) if i else np.arange(1, n)
        idx[i] = rng.choice(others, k, replace=False)
        if i:
            idx[i, rng.integers(0, k)] = 0
    sim = -np.sort(-rng.uniform(-0.2, 1.0, (n, k)), axis=1).astype(np.float32)
    if k > 1:
        for i in rng.choice(n, n // 10, replace=False):
            cut = rng.integers(1, k)
            if i:                                        # (the hub moves in front of the pads)
                at = int(np.nonzero(idx[i] == 0)[0][0])
                idx[i, at], idx[i, 0] = idx[i, 0], 0
            idx[i, cut:], sim[i, cut:] = -1, -np.inf
    if dense:
        z = np.exp(4.0 * rng.standard_normal((n, K)))    # e.g. a classifier's probabilities
        Y = (z / z.sum(1, keepdims=True)).astype(np.float32)
    else:
        Y = one_hot(np.where(np.isin(np.arange(n), rng.choice(n, max(3 * K, 20), replace=False)), rng.integers(0, K, n), -1), K)
    for a in (idx, sim, Y):
        a.setflags(write=False)
    return idx, sim, Y


@functools.lru_cache(maxsize=None)
def host_pair(n, k, K, alpha, gamma, iters, seed=0, dense=False):
    """the host's fp64 and fp32 results of a hub graph, computed once"""
    from cmlpl_amd.labelprop import labelprop_host
    idx, sim, Y = hub_graph(n, k, K, seed, dense)
    return tuple(labelprop_host(idx, sim, Y, alpha, gamma, iters, dtype=dt) for dt in (np.float64, np.float32))


QUANTITIES = ("cinv", "fwd_coef", "rev_coef", "F", "probs", "conf", "entropy")


def compare(tag, got, h64, h32):
    """the device's quantities (a dict of numpy arrays by the host's field names; ``residual`` a float) within
    tol = 8 max|host fp32 - host fp64| of the host's fp64, per quantity; labels on the sure rows; prints each figure first"""
    tol = {}
    for q in QUANTITIES + ("residual",):
        a, b = np.asarray(getattr(h32, q), np.float64), np.asarray(getattr(h64, q), np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b)), q
        tol[q] = 8 * float(np.nanmax(np.abs(a - b))) if a.size else 0.0
    F64 = np.asarray(h64.F, np.float64)
    top = -np.sort(-F64, axis=1)
    gap = top[:, 0] - top[:, 1] if F64.shape[1] > 1 else np.full(len(F64), np.inf)
    sure = gap > 2 * tol["F"]
    min_row = float(F64.sum(1).min())
    print("%s: tol_F=%.3g min_row_sum=%.3g sure=%.4f" % (tag, tol["F"], min_row, sure.mean()))
    assert sure.mean() >= 0.99 and min_row >= 1e-4
    for q in QUANTITIES + ("residual",):
        if q not in got:
            continue
        g, want = np.asarray(got[q], np.float64), np.asarray(getattr(h64, q), np.float64)
        assert g.shape == want.shape, (q, g.shape, want.shape)
        assert np.array_equal(np.isnan(g), np.isnan(want)), q
        err = float(np.nanmax(np.abs(g - want))) if g.size else 0.0
        print("  %-9s err=%.3g tol=%.3g" % (q, err, tol[q]))
        assert err <= tol[q], (q, err, tol[q])
    if "labels" in got:
        assert np.array_equal(np.asarray(got["labels"])[sure], h64.labels[sure])
    return tol
