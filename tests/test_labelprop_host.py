"""CPU: the definition of a propagated labelling restated in numpy (cmlpl_amd.labelprop.labelprop_host) on hand-made graphs
whose answers can be read off, and on the arcs, where propagation has to beat the nearest seed."""
import numpy as np
import pytest

from cmlpl_amd.labelprop import LabelProp, labelprop_host
from tests import lp_util as U

INF = np.inf


def _lp(idx, sim, Y, alpha=0.5, gamma=1, iters=1, **kw):
    return labelprop_host(np.asarray(idx, np.int32), np.asarray(sim, np.float32), np.asarray(Y, np.float32), alpha, gamma, iters, **kw)


def test_a_path_of_three_nodes():
    # 0 -> 1, 1 -> 2, 2 has no list of its own: W = A + A^T is the path 0 - 1 - 2 with weights 0.5 and 0.25
    h = _lp([[1], [2], [-1]], [[0.5], [0.25], [-INF]], [[1, 0], [0, 0], [0, 1]], alpha=0.5, iters=1)
    assert h.rev_ptr.tolist() == [0, 0, 1, 2] and h.rev_src.tolist() == [0, 1]
    d = np.array([0.5, 0.25 + 0.5, 0.25])                  # node 1: its forward edge first, then the reverse one
    assert np.allclose(h.cinv, 1 / np.sqrt(d), rtol=1e-15)
    S01, S12 = 0.5 / np.sqrt(d[0] * d[1]), 0.25 / np.sqrt(d[1] * d[2])
    assert np.allclose(h.fwd_coef[:, 0], [S01, S12, 0]) and np.allclose(h.rev_coef, [S01, S12])
    want = np.array([[0.5, 0], [0.5 * S01, 0.5 * S12], [0, 0.5]])
    assert np.allclose(h.F, want, rtol=1e-14)
    assert h.labels.tolist() == [0, 0, 1] and np.allclose(h.conf, [1, S01 / (S01 + S12), 1])
    assert np.isclose(h.residual, np.abs(want - [[1, 0], [0, 0], [0, 1]]).max())
    p = h.probs[1]
    assert np.isclose(h.entropy[1], -(p * np.log(p)).sum()) and h.entropy[0] == 0 and h.entropy[2] == 0


def test_a_mutual_pair_counts_twice():
    h = _lp([[1], [0]], [[0.5], [0.5]], [[1], [0]], gamma=2)
    assert h.rev_ptr.tolist() == [0, 1, 2] and h.rev_src.tolist() == [1, 0]
    assert np.allclose(h.cinv, 1 / np.sqrt(0.25 + 0.25))   # the pair's weight 0.5^2, once forward and once reversed
    assert np.allclose(h.fwd_coef, 0.5) and np.allclose(h.rev_coef, 0.5)
    assert np.allclose(h.F, [[0.5], [0.5 * (0.5 + 0.5) * 1.0]])


def test_a_pad_a_self_entry_and_a_negative_similarity():
    # node 0 lists itself (no edge), node 1 with a negative similarity (an edge of weight 0, kept), then a pad
    h = _lp([[0, 1, -1], [2, -1, -1], [-1, -1, -1]], [[0.9, -0.3, -INF], [0.5, -INF, -INF], [-INF] * 3], np.eye(3))
    assert h.rev_ptr.tolist() == [0, 0, 1, 2] and h.rev_src.tolist() == [0, 1]       # 0 -> 1 is in node 1's list
    assert h.cinv[0] == 0 and np.all(h.fwd_coef[0] == 0) and h.rev_coef[0] == 0       # d_0 = 0: c_0 = 0
    assert np.allclose(h.cinv[1:], 1 / np.sqrt(0.5))
    assert np.allclose(h.F, [[0.5, 0, 0], [0, 0.5, 0.5], [0, 0.5, 0.5]])
    for s in (np.nan, -INF, -1.0, 0.0):
        assert _lp([[1], [-1]], [[s], [-INF]], [[1], [1]]).rev_ptr.tolist() == [0, 0, 1]
        assert np.all(_lp([[1], [-1]], [[s], [-INF]], [[1], [1]]).cinv == 0)


def test_an_isolated_node_keeps_beta_y():
    h = _lp([[1], [0], [-1]], [[0.5], [0.5], [-INF]], [[1, 0], [0, 0], [0.25, 0.75]], alpha=0.75, iters=7)
    assert h.cinv[2] == 0 and h.F[2].tolist() == [0.25 * 0.25, 0.25 * 0.75] and h.labels[2] == 1
    assert np.allclose(h.probs[2], [0.25, 0.75])


def test_a_component_without_a_seed_is_unreached():
    h = _lp([[1], [0], [3], [2]], [[0.5]] * 4, [[1, 0], [0, 0], [0, 0], [0, 0]], alpha=0.9, iters=30)
    assert h.labels.tolist() == [0, 0, -1, -1]
    assert np.isnan(h.probs[2:]).all() and np.isnan(h.conf[2:]).all() and np.isnan(h.entropy[2:]).all()
    assert not np.isnan(h.probs[:2]).any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_alpha_zero_gives_the_bytes_of_y(dtype):
    idx, sim, Y = U.hub_graph(60, 4, 5)
    for iters in (1, 3):
        h = labelprop_host(idx, sim, Y, 0.0, 3, iters, dtype=dtype)
        assert h.F.astype(np.float32).tobytes() == Y.tobytes()
    assert h.residual == 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ten_and_ten_iterations_are_twenty(dtype):
    idx, sim, Y = U.hub_graph(60, 4, 5)
    if dtype is np.float64:                                # (F0 is taken as fp32, as the device's is: compare in fp32 only)
        a = labelprop_host(idx, sim, Y, 0.9, 3, 10, dtype=np.float32)
        b = labelprop_host(idx, sim, Y, 0.9, 3, 10, F0=a.F, dtype=np.float64)
        assert np.abs(b.F - labelprop_host(idx, sim, Y, 0.9, 3, 20).F).max() < 1e-6
        return
    a = labelprop_host(idx, sim, Y, 0.9, 3, 10, dtype=dtype)
    b = labelprop_host(idx, sim, Y, 0.9, 3, 10, F0=a.F, dtype=dtype)
    c = labelprop_host(idx, sim, Y, 0.9, 3, 20, dtype=dtype)
    assert b.F.tobytes() == c.F.tobytes() and b.residual == c.residual and np.array_equal(b.labels, c.labels)


def test_reverse_lists_are_in_ascending_source_order():
    idx, sim, Y = U.hub_graph(200, 5, 3)
    h = labelprop_host(idx, sim, Y, 0.9, 3, 1)
    assert h.rev_ptr[-1] == ((idx >= 0) & (idx != np.arange(200)[:, None])).sum()
    assert h.rev_ptr[1] - h.rev_ptr[0] == 199                                            # the hub
    for i in range(200):
        src = h.rev_src[h.rev_ptr[i]:h.rev_ptr[i + 1]]
        assert np.all(np.diff(src) >= 0) and sorted(src.tolist()) == sorted(np.nonzero((idx == i).any(1))[0].tolist())


def test_the_ranges_are_checked():
    idx, sim, Y = U.hub_graph(60, 4, 5)
    for kw in (dict(alpha=1.0), dict(alpha=-0.1), dict(gamma=0), dict(gamma=9), dict(iters=0), dict(iters=10001)):
        with pytest.raises(ValueError):
            labelprop_host(idx, sim, Y, **{**dict(alpha=0.5, gamma=3, iters=1), **kw})
    for cfg in (LabelProp(k=0), LabelProp(k=33), LabelProp(alpha=1.0), LabelProp(gamma=9), LabelProp(iters=0)):
        with pytest.raises(ValueError):
            cfg.check()
    assert LabelProp().check() == (10, 0.99, 3, 50)


@pytest.mark.parametrize("n_per,dphi,k", U.ARC_CASES)
def test_on_the_arcs_propagation_beats_the_nearest_seed(n_per, dphi, k):
    """Measured with the draws in the order written (tests/lp_util.py): nearest seed 0.756 / 0.700, propagated 0.896 / 0.931
    -- lifts of 0.14 and 0.23."""
    X, truth, seeds = U.arcs(n_per, dphi)
    idx, sim = U.exact_neighbours(X, k)
    h = labelprop_host(idx, sim, U.one_hot(seeds, 9), U.ARC_ALPHA, U.ARC_GAMMA, U.ARC_ITERS)
    near, got = U.nearest_seed_accuracy(X, truth, seeds), float((h.labels == truth).mean())
    print("arcs n=%d k=%d: nearest seed %.3f, propagated %.3f" % (len(truth), k, near, got))
    assert (h.labels >= 0).all()
    assert got >= near + 0.10


def test_the_drivers_refuse_what_propagate_cannot_mean():
    import predict
    import train

    def refused(mod, argv, word):
        args = mod.build_parser().parse_args(argv)
        with pytest.raises(SystemExit) as e:
            if mod is predict:
                predict.check_args(args), predict.check_knn_args(args), predict.check_propagate_args(args)
            else:
                train.propagate_of(args)
        assert word in str(e.value), (argv, str(e.value))

    ck = ["--ckpt", "x.pt"]
    for extra, word in ((["--net", "ensemble", "--propagate"], "ONE network"), (["--net", "ensemble_all", "--propagate"], "ONE network"),
                        (["--lp_k", "5"], "belongs to --propagate"), (["--lp_alpha", "0.5", "--lp_iters", "3"], "belong to --propagate"),
                        (["--propagate", "--out", "x.npy"], "not the scene"), (["--propagate", "--proba", "x.npy"], "not the scene"),
                        (["--propagate", "--confidence", "x.npy"], "not the scene"), (["--propagate", "--entropy", "x.npy"], "not the scene"),
                        (["--propagate", "--tta", "2"], "not the scene"), (["--propagate", "--smooth", "2"], "not the scene"),
                        (["--propagate", "--temperature", "2"], "not the scene"), (["--propagate", "--lp_k", "33"], "--lp_k"),
                        (["--propagate", "--lp_alpha", "1"], "--lp_alpha"), (["--propagate", "--lp_gamma", "0"], "--lp_gamma"),
                        (["--propagate", "--lp_iters", "0"], "--lp_iters")):
        refused(predict, ck + extra, word)
    for extra, word in ((["--lp_gamma", "2"], "belongs to --propagate"), (["--propagate", "--lp_k", "0"], "--lp_k"),
                        (["--propagate", "--lp_iters", "10001"], "--lp_iters")):
        refused(train, extra, word)
    for mod, argv in ((predict, ck + ["--propagate", "--net", "both", "--knn", "5"]), (predict, ck + ["--propagate", "--reliability"]),
                      (train, ["--propagate", "--lp_k", "4", "--lp_alpha", "0", "--lp_gamma", "8", "--lp_iters", "10000"])):
        args = mod.build_parser().parse_args(argv)
        if mod is predict:
            predict.check_args(args), predict.check_knn_args(args), predict.check_propagate_args(args)
        assert train.propagate_of(args) is not None
    # the flag is never recorded in a checkpoint: a run with it writes the bytes of a run without
    a, b = (train.build_parser().parse_args(v) for v in (["--propagate", "--lp_k", "4"], []))
    assert train.saved_args(a) == train.saved_args(b)


def test_train_refuses_propagate_on_several_ranks(monkeypatch):
    import train
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:                   # (before any device or communicator work)
        train.main(train.build_parser().parse_args(["--synthetic", "B2", "--propagate"]))
    assert "--propagate runs on one GPU" in str(e.value)


def test_score_labels_counts_an_unreached_row_as_wrong():
    from cmlpl_amd.labelprop import score_labels
    OA, Kappa, producerA, AA, cm = score_labels([0, 1, -1, 1, 2, -1], [0, 1, 1, 1, 2, 0], 3)
    assert cm.tolist() == [[1, 0, 0, 1], [0, 2, 0, 1], [0, 0, 1, 0]]
    assert np.isclose(OA, 4 / 6) and np.allclose(producerA, [0.5, 2 / 3, 1]) and np.isclose(AA, (0.5 + 2 / 3 + 1) / 3)
    pe = (1 * 2 + 2 * 3 + 1 * 1) / 36
    assert np.isclose(Kappa, (4 / 6 - pe) / (1 - pe))
