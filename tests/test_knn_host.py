"""CPU: ``cmlpl_amd.knn.knn_host`` / ``vote_host`` -- the numpy restatement of include/cmlpl.h, "THE DEFINITION OF A kNN
VOTE", which tests/test_gpu_knn.py holds the kernel to -- on hand-made cases whose answers can be read off."""
import numpy as np
import pytest

from cmlpl_amd.knn import KnnResult, knn_host, purity, vote_host

D = 1024


def _rows(*vals):
    """rows whose similarity with the unit query e_0 is the given value (the value in column 0)"""
    r = np.zeros((len(vals), D), np.float32)
    r[:, 0] = vals
    return r


def _e0(n=1):
    q = np.zeros((n, D), np.float32)
    q[:, 0] = 1.0
    return q


def test_equal_similarities_go_by_index_and_zeros_of_either_sign_are_equal():
    g = _rows(0.5, 0.75, 0.5, 0.75, 0.5)
    h = knn_host(_e0(), g, np.zeros(5, np.int64), 1, 4)
    assert h.nbr_idx.tolist() == [[1, 3, 0, 2]]
    assert h.nbr_sim.tolist() == [[0.75, 0.75, 0.5, 0.5]]
    g = _rows(-0.0, 0.0, -0.0, 0.0)
    h = knn_host(_e0(), g, np.zeros(4, np.int64), 1, 3)
    assert h.nbr_idx.tolist() == [[0, 1, 2]]


def test_skip_takes_one_gallery_row_out_per_query():
    g = _rows(0.9, 0.8, 0.7)
    lab = np.array([0, 1, 2])
    h = knn_host(_e0(3), g, lab, 3, 2, skip=np.array([0, -1, 2]))
    assert h.nbr_idx.tolist() == [[1, 2], [0, 1], [0, 1]]
    assert h.labels.tolist() == [1, 0, 0]


def test_gallery_labels_out_of_range_are_never_neighbours():
    g = _rows(0.9, 0.8, 0.7, 0.6)
    h = knn_host(_e0(), g, np.array([-1, 3, 1, 0]), 3, 3)
    assert h.nbr_idx.tolist() == [[2, 3, -1]]


def test_fewer_candidates_than_k():
    g = _rows(0.25, 0.5)
    h = knn_host(_e0(), g, np.array([1, 0]), 2, 4, T=1.0)
    assert h.nbr_idx.tolist() == [[1, 0, -1, -1]]
    assert h.nbr_sim[0, :2].tolist() == [0.5, 0.25] and np.isneginf(h.nbr_sim[0, 2:]).all()
    w1 = np.exp(-0.25)                                 # the missing ranks weigh 0
    np.testing.assert_allclose(h.probs[0], [1 / (1 + w1), w1 / (1 + w1)], rtol=1e-12)
    np.testing.assert_allclose(h.probs32[0], h.probs[0], rtol=1e-6)
    assert h.probs32.dtype == np.float32 and h.labels.tolist() == [0] and h.labels32.tolist() == [0]


def test_a_nan_query_has_no_candidate_and_a_nan_gallery_row_is_never_chosen():
    q = _e0(2)
    q[1, 5] = np.nan
    g = _rows(0.5, 0.9, 0.7)
    g[1, 7] = np.nan
    h = knn_host(q, g, np.array([0, 1, 1]), 2, 2)
    assert h.nbr_idx.tolist() == [[2, 0], [-1, -1]]
    assert h.labels.tolist() == [1, -1] and h.labels32.tolist() == [1, -1]
    assert np.isnan(h.probs[1]).all() and np.isnan(h.probs32[1]).all() and not np.isnan(h.probs[0]).any()
    assert np.isneginf(h.nbr_sim[1]).all()


def test_k_1_is_the_nearest_rows_label():
    rng = np.random.Generator(np.random.PCG64(1))
    q, g = rng.standard_normal((7, D)).astype(np.float32), rng.standard_normal((20, D)).astype(np.float32)
    lab = rng.integers(0, 5, 20)
    h = knn_host(q, g, lab, 5, 1, T=0.07)
    near = (q.astype(np.float64) @ g.astype(np.float64).T).argmax(1)
    assert h.nbr_idx[:, 0].tolist() == near.tolist() and h.labels.tolist() == lab[near].tolist()
    assert np.array_equal(h.probs, np.eye(5)[lab[near]]) and np.array_equal(h.probs32, np.eye(5, dtype=np.float32)[lab[near]])


def test_a_very_large_T_is_the_unweighted_majority_with_first_maximum_ties():
    g = _rows(0.9, 0.8, 0.7, 0.6, 0.5, 0.4)
    h = knn_host(_e0(), g, np.array([2, 1, 1, 2, 0, 0]), 3, 4, T=1e30)          # classes 1 and 2 tie 2 : 2
    assert h.probs[0].tolist() == [0.0, 0.5, 0.5] and h.labels.tolist() == [1] and h.labels32.tolist() == [1]
    h = knn_host(_e0(), g, np.array([2, 1, 1, 2, 0, 0]), 3, 5, T=1e30)
    assert h.probs32[0].tolist() == [np.float32(0.2), np.float32(0.4), np.float32(0.4)]


def test_the_search_alone_without_labels():
    g = _rows(0.1, 0.3, 0.2)
    h = knn_host(_e0(), g, None, 0, 2)
    assert h.nbr_idx.tolist() == [[1, 2]] and h.probs is None and h.labels is None


def test_vote_host_weights_follow_the_chain():
    idx = np.array([[3, 0, 1]])
    sim = np.array([[0.8, 0.6, 0.1]])
    lab = np.array([1, 0, 9, 1])
    p64, l64, p32, l32 = vote_host(idx, sim, lab, 2, 0.1)
    inv = float(np.float32(1.0 / 0.1))
    w = np.exp((sim[0] - sim[0, 0]) * inv)
    np.testing.assert_allclose(p64[0], [w[2] / w.sum(), (w[0] + w[1]) / w.sum()], rtol=1e-14)
    s32 = sim.astype(np.float32)[0]
    w32 = np.exp(((s32 - s32[0]) * np.float32(inv)).astype(np.float32)).astype(np.float32)
    den = np.float32(np.float32(w32[0] + w32[1]) + w32[2])
    assert w32[0] == 1.0 and p32[0].tolist() == [np.float32(w32[2] / den), np.float32(np.float32(w32[0] + w32[1]) / den)]
    assert l64.tolist() == [1] and l32.tolist() == [1]


def test_purity():
    idx = np.array([[0, 1, 2], [2, 3, -1], [-1, -1, -1]], np.int32)
    lab = np.array([0, 0, 1, 2])
    truth = np.array([0, 1, 0])
    assert purity(idx, lab, truth) == pytest.approx((2 / 3 + 1 / 2) / 2)        # the query without a neighbour is left out
    res = KnnResult(None, None, idx, None)
    assert res.purity(lab, truth) == purity(idx, lab, truth)
    with pytest.raises(ValueError):
        KnnResult(None, None, None, None).purity(lab, truth)


def test_ranges():
    with pytest.raises(ValueError):
        knn_host(_e0(), _rows(0.1), np.array([0]), 1, 33)
    with pytest.raises(ValueError):
        knn_host(_e0(), _rows(0.1), np.array([0]), 65, 1)
    with pytest.raises(ValueError):
        knn_host(_e0(), _rows(0.1), np.array([0]), 1, 1, T=0.0)
