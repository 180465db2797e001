"""CPU: the definitions of a region descriptor, a region adjacency and a region graph as cmlpl_amd.regiongraph restates them
(pool_host, adjacency_host, merge_lists_host, region_graph_host) -- against brute force on tiny maps, against the invariants
the header states, and on the case builder of tests/test_smooth_host.py, where the stage's accuracy can never exceed the
achievable segmentation accuracy of the map it runs on."""
import os

import numpy as np
import pytest

from cmlpl_amd.regiongraph import (RegionGraph, adjacency_host, contacts_host, merge_lists_host, pool_host, region_graph_host)
from tests.regions_cases import pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = [("random9", 5, 7, 9), ("voids", 6, 5, 2), ("stripes_h", 4, 9, 2), ("checker", 5, 5, 2), ("constant", 3, 4, 6),
        ("comb", 7, 8, 4), ("random9", 1, 12, 9), ("random9", 12, 1, 9), ("random9", 1, 1, 9)]


def brute_adjacency(ids, M, rows, cols):
    b = np.zeros((M, M), np.int64)
    inside = lambda v: 0 <= v < M
    for y in range(rows):
        for x in range(cols):
            p = int(ids[y * cols + x])
            for dy, dx in ((0, 1), (1, 0)):
                if y + dy < rows and x + dx < cols:
                    q = int(ids[(y + dy) * cols + x + dx])
                    if inside(p) and inside(q) and p != q:
                        b[p, q] += 1
                        b[q, p] += 1
    return b


@pytest.mark.parametrize("name,rows,cols,M", MAPS)
def test_adjacency_against_brute_force_and_its_invariants(name, rows, cols, M):
    ids = pattern(name, rows, cols, 7)
    b = brute_adjacency(ids, M, rows, cols)
    assert np.array_equal(b, b.T)                                                    # b[s][t] == b[t][s]
    contacts = len(contacts_host(ids, M, rows, cols)[0])
    for A in (0, 1, 3, 16):
        adj = adjacency_host(ids, M, rows, cols, A)
        assert adj["adj_idx"].shape == adj["adj_len"].shape == (M, A)
        assert np.array_equal(adj["deg"], (b > 0).sum(1)) and np.array_equal(adj["boundary"], b.sum(1))
        assert int(adj["boundary"].sum()) == 2 * contacts                            # sum_s boundary[s] = 2 x the contacts
        for s in range(M):
            want = sorted((t for t in range(M) if b[s, t] > 0), key=lambda t: (-b[s, t], t))[:A]
            got = adj["adj_idx"][s]
            assert got[:len(want)].tolist() == want and (got[len(want):] == -1).all()
            assert adj["adj_len"][s, :len(want)].tolist() == [b[s, t] for t in want] and (adj["adj_len"][s, len(want):] == 0).all()
            assert (got >= 0).sum() == min(A, adj["deg"][s])                         # deg and the list agree below the cut


def test_a_known_small_map_with_a_tie_a_void_and_an_id_past_m():
    ids = np.array([[0, 0, 1],
                    [2, 0, 1],
                    [2, -1, 7]], np.int32).reshape(-1)
    adj = adjacency_host(ids, 3, 3, 3, 2)                        # (7 >= M: void)
    assert adj["adj_idx"].tolist() == [[1, 2], [0, -1], [0, -1]]          # region 0 touches 1 twice and 2 twice: the smaller id first
    assert adj["adj_len"].tolist() == [[2, 2], [2, 0], [2, 0]]
    assert adj["deg"].tolist() == [2, 1, 1] and adj["boundary"].tolist() == [4, 2, 2]
    one = adjacency_host(ids, 3, 3, 3, 1)
    assert one["adj_idx"].tolist() == [[1], [0], [0]] and one["deg"].tolist() == [2, 1, 1]        # truncated, deg is not


def test_pool_against_brute_force():
    rng = np.random.default_rng(3)
    n, B, M = 40, 5, 6
    ids = rng.integers(-1, M + 2, n).astype(np.int32)
    ids[ids == 4] = 3                                            # region 4 is empty
    X = rng.standard_normal((n, B)).astype(np.float32)
    X[1, 2], X[2, 0], X[3, 4], X[4, 1], X[5, 3], X[6, 0], X[7, 2] = np.nan, np.inf, -np.inf, 256.0, -256.0, 257.0, 2.0 ** -30
    got = pool_host(ids, M, X)
    S, cnt = np.zeros((M, B), object), np.zeros(M, np.int64)
    for p in range(n):
        s = int(ids[p])
        if not 0 <= s < M or not all(np.isfinite(v) and abs(float(v)) <= 256.0 for v in X[p]):
            continue
        cnt[s] += 1
        for b in range(B):
            S[s, b] += int(round(float(X[p, b]) * 2 ** 24))      # (Python rounds halves to even, as llrintf does)
    assert np.array_equal(got["cnt"], cnt) and np.array_equal(got["S"], S.astype(np.int64))
    assert cnt[4] == 0 and (got["mean"][4] == 0).all()
    for s in range(M):
        if cnt[s]:
            want = np.array([np.float32(float(S[s, b]) / (float(cnt[s]) * 2.0 ** 24)) for b in range(B)], np.float32)
            assert got["mean"][s].tobytes() == want.tobytes()
    pooled = {p for p in range(n) if 0 <= ids[p] < M} - {1, 2, 3, 6}
    assert int(cnt.sum()) == len(pooled)                         # 256 and -256 are pooled, 257 is not
    if 0 <= ids[7] < M:
        lone = pool_host(ids[7:8], M, X[7:8])
        assert lone["S"][ids[7], 2] == 0                         # 2^-30 rounds to 0


def test_merged_lists_against_brute_force():
    rng = np.random.default_rng(5)
    M, k, A = 7, 2, 3
    feat = rng.standard_normal((M, 1024)).astype(np.float32)
    feat[5] = np.nan
    knn_idx = np.array([[1, 2], [0, -1], [0, 3], [2, 4], [3, -1], [-1, -1], [4, 0]], np.int32)
    knn_sim = np.where(knn_idx >= 0, rng.random((M, k)), -np.inf)
    adj_idx = np.array([[1, 3, -1], [0, 2, 5], [1, -1, -1], [2, 0, 4], [-1, -1, -1], [1, 6, -1], [5, 9, -1]], np.int32)
    idx, sim = merge_lists_host(feat, knn_idx, knn_sim, adj_idx)
    assert idx.shape == sim.shape == (M, k + A)
    assert np.array_equal(idx[:, :k], knn_idx) and np.array_equal(sim[:, :k], knn_sim)
    f = feat.astype(np.float64)
    for s in range(M):
        for a in range(A):
            t = int(adj_idx[s, a])
            if t < 0 or t >= M or t in knn_idx[s]:
                assert idx[s, k + a] == -1 and sim[s, k + a] == -np.inf
            else:
                assert idx[s, k + a] == t
                want = float(np.dot(f[s], f[t]))
                assert (np.isnan(want) and np.isnan(sim[s, k + a])) or abs(sim[s, k + a] - want) <= 1e-9 * max(1.0, abs(want))
    assert idx[0].tolist() == [1, 2, -1, 3, -1] and idx[6, k:].tolist() == [5, -1, -1]        # present in both; an id past M
    assert np.isnan(sim[6, k])                                   # a NaN row's dot product is stored as it is
    only_adj = merge_lists_host(feat, None, None, adj_idx)
    assert only_adj[0].shape == (M, A) and only_adj[0][0].tolist() == [1, 3, -1]
    only_knn = merge_lists_host(feat, knn_idx, knn_sim, None)
    assert np.array_equal(only_knn[0], knn_idx)


@pytest.mark.parametrize("rows,cols,K,G", [(37, 29, 9, 3), (61, 47, 9, 3)])
def test_the_stage_never_exceeds_the_achievable_segmentation_accuracy(rows, cols, K, G):
    """7-pixel regions, S = 4, the soft vote, unit-length region descriptors made from the mean guide.  OA_rg <= ASA is a
    true bound (a region carries one label); the vote's OA and the stage's OA are printed as measured, whichever way they
    fall: no lift is promised."""
    from cmlpl_amd.superpixel import asa, region_vote_host, segment_host
    from tests.test_smooth_host import case
    p, cube, Y = case(rows, cols, K, G, 1)
    n = rows * cols
    segs = segment_host(cube, 4, 1.0, 10, G)
    seg, N = segs["seg"], segs["ny"] * segs["nx"]
    vote = region_vote_host(seg, N, K, probs=p)
    pooled = pool_host(seg, N, cube.reshape(n, -1)[:, :G])
    feat = np.zeros((N, 1024), np.float32)
    feat[:, :G] = pooled["mean"]
    with np.errstate(all="ignore"):
        feat = (feat / np.linalg.norm(feat.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    feat[pooled["cnt"] == 0] = np.nan
    out = region_graph_host(seg, N, rows, cols, feat, vote["q"], RegionGraph())
    bound = asa(seg, N, np.arange(n), Y, K)
    oa_raw, oa_vote, oa_rg = (p.argmax(1) == Y).mean(), (vote["labels"] == Y).mean(), (out["labels"] == Y).mean()
    print("%d x %d x %d: OA pixels %.4f, vote %.4f, region graph %.4f, ASA %.4f (%d regions, %d unreached)" % (
        rows, cols, K, oa_raw, oa_vote, oa_rg, bound, N, int((out["lp"].labels < 0).sum())))
    assert oa_rg <= bound + 1e-12 and oa_vote <= bound + 1e-12
    inside = (seg >= 0) & (seg < N)
    assert np.array_equal(out["labels"][inside], out["lp"].labels[seg[inside]])      # a pixel takes its region's label
    zero = region_graph_host(seg, N, rows, cols, feat, vote["q"], RegionGraph(alpha=0.0))
    assert np.array_equal(zero["labels"], vote["labels"])                            # alpha = 0 returns the vote's labels
    seeds = (np.arange(0, n, 5), Y[::5])
    seeded = region_graph_host(seg, N, rows, cols, feat, vote["q"], RegionGraph(), seeds=seeds)
    hist = region_vote_host(seg, N, K, labels=np.where(np.isin(np.arange(n), seeds[0]), Y, -1))
    has = hist["cnt"] > 0
    assert has.any() and np.array_equal(seeded["Y"][has], hist["q"][has]) and np.array_equal(seeded["Y"][~has], out["Y"][~has])


def test_region_graph_validation():
    assert RegionGraph() == (8, 8, 0.5, 3, 20, 0) and RegionGraph().check(2) == RegionGraph()
    assert RegionGraph(k=0, adj=1).check() and RegionGraph(k=32, adj=0).check() and RegionGraph(k=16, adj=16).check()
    for bad in (RegionGraph(k=0, adj=0), RegionGraph(k=17, adj=16), RegionGraph(k=-1), RegionGraph(adj=17), RegionGraph(alpha=1.0),
                RegionGraph(alpha=float("nan")), RegionGraph(gamma=0), RegionGraph(gamma=9), RegionGraph(iters=0), RegionGraph(net=-1)):
        with pytest.raises(ValueError):
            bad.check()
    with pytest.raises(ValueError):
        RegionGraph(net=2).check(2)


def test_the_source_is_built_and_the_header_declares_the_exports():
    from cmlpl_amd import _lib, build_ext
    names = ("cmlpl_rg_workspace_bytes", "cmlpl_rg_pool", "cmlpl_rg_adjacency", "cmlpl_rg_lists")
    assert build_ext.SOURCES[-2:] == ["regions.hip", "regiongraph.hip"] and all(n in _lib.EXPORTS for n in names)
    header = open(os.path.join(ROOT, "include", "cmlpl.h")).read()
    assert all(n + "(" in header for n in names)
    for what in ("A REGION DESCRIPTOR", "A REGION ADJACENCY", "A REGION GRAPH"):
        assert "THE DEFINITION OF " + what in header
    import cmlpl_amd
    assert cmlpl_amd.RegionGraph is RegionGraph and cmlpl_amd.pool_host is pool_host


def test_parsers_take_the_flags_and_refuse_what_they_cannot_mean():
    import predict
    import train
    from scene_report import Stage, region_graph_stage
    tp, pp = train.build_parser(), predict.build_parser()
    a = tp.parse_args(["--superpixel", "4", "--region_graph", "--rg_k", "4", "--rg_adj", "6", "--rg_alpha", "0.3", "--rg_net", "1"])
    assert train.region_graph_of(a, 2) == RegionGraph(4, 6, 0.3, net=1)
    assert train.region_graph_of(tp.parse_args(["--superpixel", "4", "--region_graph"])) == RegionGraph()
    assert train.region_graph_of(tp.parse_args([])) is None
    saved = train.saved_args(a)
    assert not any(k.startswith(("rg_", "region_graph")) for k in saved) and saved == train.saved_args(tp.parse_args([]))
    for argv, word in ((["--region_graph"], "belongs to --superpixel"), (["--rg_k", "3"], "belongs to --region_graph"),
                       (["--superpixel", "4", "--rg_adj", "3", "--rg_iters", "5"], "belong to --region_graph"),
                       (["--superpixel", "4", "--region_graph", "--rg_k", "0", "--rg_adj", "0"], "k + adj 1 .. 32"),
                       (["--superpixel", "4", "--region_graph", "--rg_k", "30", "--rg_adj", "3"], "k + adj 1 .. 32"),
                       (["--superpixel", "4", "--region_graph", "--rg_net", "2"], "net names no member")):
        with pytest.raises(SystemExit) as e:
            train.region_graph_of(tp.parse_args(argv), 2)
        assert word in str(e.value), argv
    base = ["--ckpt", "x.pt"]
    for argv, word in ((["--net", "both", "--superpixel", "4", "--region_graph"], "--region_graph gives ONE prediction"),
                       (["--net", "ema_both", "--superpixel", "4", "--region_graph"], "--net ema_both"),
                       (["--net", "ensemble", "--region_graph"], "belongs to --superpixel"),
                       (["--net", "ensemble", "--superpixel", "4", "--rg_gamma", "2"], "belongs to --region_graph"),
                       (["--net", "0", "--superpixel", "4", "--region_graph", "--rg_net", "1"], "net names no member"),
                       (["--net", "ensemble", "--superpixel", "4", "--region_graph", "--rg_net", "2"], "net names no member"),
                       (["--net", "ensemble", "--superpixel", "4", "--region_graph", "--rg_k", "20", "--rg_adj", "13"], "k + adj 1 .. 32")):
        with pytest.raises(SystemExit) as e:
            predict.check_args(pp.parse_args(base + argv))
        assert word in str(e.value), argv
    ok = pp.parse_args(base + ["--net", "ensemble", "--smooth", "2", "--superpixel", "4", "--region_graph", "--rg_net", "1",
                               "--temperature", "2", "--sieve", "4"])
    predict.check_args(ok)
    assert [name for name, _ in predict.plan(ok, True).stages] == ["smooth", "superpixel", "region_graph", "temper", "sieve"]
    assert predict.plan(pp.parse_args(base + ["--net", "ensemble", "--superpixel", "4"]), True).stages[0][0] == "superpixel"
    stage = region_graph_stage(RegionGraph())
    assert stage.suffix == "_rg" and stage.scored is True and stage.scene is True and Stage("t", "_x", None).scene is False


def test_the_end_to_end_case_meets_the_comparisons_own_conditions_on_the_host():
    """tests/test_gpu_regiongraph.py compares the device with the host through tests/lp_util.compare, which first asserts for
    the host alone that at least 99 % of the rows are sure and no fp64 row sum is below 1e-4: the seeded case is held to
    that here, with the embedding restated on the host (the device's lists differ from these in the last bits only)."""
    from cmlpl_amd.superpixel import region_vote_host, segment_host
    from tests import lp_util as U
    from tests.regiongraph_cases import E2E, e2e_case, embed_host
    c = e2e_case()
    rows, cols, K = E2E["rows"], E2E["cols"], E2E["K"]
    segs = segment_host(c["cube"], E2E["step"], 1.0, 10, E2E["G"])
    seg, N = segs["seg"], segs["ny"] * segs["nx"]
    vote = region_vote_host(seg, N, K, probs=c["p"])
    pooled = pool_host(seg, N, c["spectra"])
    feat = embed_host(c["params"], pooled["mean"])
    feat[pooled["cnt"] == 0] = np.nan
    assert 100 <= N <= 1000 and not np.isnan(feat).any()
    for cfg in (RegionGraph(), RegionGraph(k=4, adj=4, alpha=0.9, iters=50)):
        h64 = region_graph_host(seg, N, rows, cols, feat, vote["q"], cfg)
        h32 = region_graph_host(seg, N, rows, cols, feat, vote["q"], cfg, lists=(h64["nbr_idx"], h64["nbr_sim"]), dtype=np.float32)
        U.compare("host %s" % (cfg,), {}, h64["lp"], h32["lp"])
