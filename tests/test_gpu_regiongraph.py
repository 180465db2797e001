"""GPU: cmlpl_rg_pool / cmlpl_rg_adjacency / cmlpl_rg_lists (csrc/regiongraph.hip) against the host's restatements of the
header's definitions -- the pool bit for bit, the adjacency exactly, the merged lists exactly in their indices and inside the
standard bound of a length-1024 fp32 dot product in their similarities -- and the stage end to end: the host's definition
evaluated on the device's lists, through tests/lp_util.compare with its allowances unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from cmlpl_amd.regiongraph import (RegionGraph, adjacency, adjacency_host, merge_lists, merge_lists_host, pool, pool_host,
                                   region_graph, region_graph_host, region_propagate)
from tests import lp_util as U
from tests.gpu_util import DEV
from tests.regiongraph_cases import E2E, e2e_case, region_map

pytestmark = pytest.mark.gpu

POOL_SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (61, 47)]
POOL_MAPS = ("pixels", "one", "components", "voids", "past_M", "empty")
ADJ_SHAPES = [(1, 1), (1, 70), (70, 1), (3, 50), (33, 65), (64, 64), (65, 65), (61, 47), (96, 96)]
ADJ_MAPS = ("constant", "pixels", "stripes_h", "stripes_v", "spiral", "comb", "smoothed_components", "voids", "hub")
SPECIAL = (np.nan, np.inf, -np.inf, 256.0, -256.0, 257.0, 2.0 ** -30)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)                 # (a copy: the shared inputs are read-only)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def pool_input(n, B, seed=0):
    """X [n, B] of N(0, 1) with each special value at about one element in 40 rows (n = 1: a clean row), and the rows that
    hold 256 / -256 / 2^-30 only: they are pooled"""
    rng = np.random.default_rng(100 * B + seed)
    X = rng.standard_normal((n, B)).astype(np.float32)
    if n > 1:
        for v in SPECIAL:
            at = rng.integers(0, n, max(1, n // 40))
            X[at, rng.integers(0, B, len(at))] = v
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("B", [1, 60, 103, 204])
@pytest.mark.parametrize("rows,cols", POOL_SHAPES)
def test_the_pool_is_the_definition_bit_for_bit(rows, cols, B):
    n = rows * cols
    X = pool_input(n, B)
    wide = torch.full((n, B + 5), float("nan"), device=DEV)                          # a row stride larger than B
    wide[:, :B] = _dev(X)
    for name in POOL_MAPS:
        ids, M = region_map(name, rows, cols)
        ref = pool_host(ids, M, X)
        for src in (_dev(X), wide[:, :B]):
            got = pool(_dev(ids), M, src, sums=True)
            assert got.mean.cpu().numpy().tobytes() == ref["mean"].tobytes(), (name, "mean")
            assert np.array_equal(got.cnt.cpu().numpy(), ref["cnt"]), (name, "cnt")
            assert np.array_equal(got.S.cpu().numpy(), ref["S"]), (name, "S")
        if name == "empty":
            assert (ref["cnt"] == 0).any()
    without = pool(_dev(ids), M, _dev(X))                                             # S is optional
    assert without.S is None and without.mean.cpu().numpy().tobytes() == ref["mean"].tobytes()


def test_the_pool_takes_the_edges_of_its_range_and_both_region_paths():
    """256 and -256 are pooled, 257 and every non-finite value is not, 2^-30 rounds to 0; a region of exactly 64 pixels is
    a wavefront's, one of 65 a workgroup's"""
    B = 3
    X = np.zeros((8, B), np.float32)
    X[0], X[1], X[2], X[3], X[4], X[5], X[6] = 256.0, -256.0, 257.0, np.nan, np.inf, 2.0 ** -30, -np.inf
    X[7] = 0.5
    ids = np.zeros(8, np.int32)
    got = pool(_dev(ids), 1, _dev(X), sums=True)
    assert int(got.cnt[0]) == 4 and got.S[0].tolist() == [2 ** 23] * 3               # 256 - 256 + 0 + 0.5, times 2^24
    ref = pool_host(ids, 1, X)
    assert got.mean.cpu().numpy().tobytes() == ref["mean"].tobytes() and np.array_equal(got.S.cpu().numpy(), ref["S"])
    for size in (63, 64, 65, 129):
        n = size + 70
        ids = np.concatenate([np.zeros(size, np.int32), np.ones(70, np.int32)])[np.random.default_rng(size).permutation(n)]
        X = pool_input(n, 103, size)
        got, ref = pool(_dev(ids), 2, _dev(X), sums=True), pool_host(ids, 2, X)
        assert np.array_equal(got.S.cpu().numpy(), ref["S"]) and np.array_equal(got.cnt.cpu().numpy(), ref["cnt"]), size
        assert got.mean.cpu().numpy().tobytes() == ref["mean"].tobytes(), size


@functools.lru_cache(maxsize=None)
def adjacency_ref(name, rows, cols):
    ids, M = region_map(name, rows, cols)
    return adjacency_host(ids, M, rows, cols, 16)                                    # (a shorter list is its prefix)


@pytest.mark.parametrize("A", [0, 1, 4, 16])
@pytest.mark.parametrize("rows,cols", ADJ_SHAPES)
def test_the_adjacency_is_the_definition_exactly(rows, cols, A):
    for name in ADJ_MAPS:
        ids, M = region_map(name, rows, cols)
        ref = adjacency_ref(name, rows, cols)
        got = adjacency(_dev(ids), M, rows, cols, A)
        assert got.adj_idx.shape == got.adj_len.shape == (M, A)
        assert np.array_equal(got.deg.cpu().numpy(), ref["deg"]), (name, "deg")
        assert np.array_equal(got.boundary.cpu().numpy(), ref["boundary"]), (name, "boundary")
        assert np.array_equal(got.adj_idx.cpu().numpy(), ref["adj_idx"][:, :A]), (name, "adj_idx")
        assert np.array_equal(got.adj_len.cpu().numpy(), ref["adj_len"][:, :A]), (name, "adj_len")
        if name == "constant":
            assert int(ref["boundary"].sum()) == 0
        if name == "hub" and rows >= 33 and cols >= 33:
            assert ref["deg"][0] > 100 and ref["deg"][0] > 16                         # truncated, with ties to the smaller id
            assert (np.diff(ref["adj_idx"][0]) > 0).all() and (ref["adj_len"][0] == ref["adj_len"][0, 0]).all()


def lists_case(M=70, k=5, A=6, seed=0):
    """feat [M, 1024] with NaN rows, arbitrary kNN lists with pads, and adjacency lists that repeat kNN entries in both
    directions, hold pads and name NaN rows"""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((M, 1024)).astype(np.float32)
    feat /= np.linalg.norm(feat, axis=1, keepdims=True)
    feat[[3, M - 2]] = np.nan
    knn_idx = np.stack([rng.choice(np.delete(np.arange(M), s), k, replace=False) for s in range(M)]).astype(np.int32)
    knn_sim = -np.sort(-rng.uniform(-0.2, 1.0, (M, k)), axis=1).astype(np.float32)
    knn_idx[5, 2:], knn_sim[5, 2:] = -1, -np.inf
    adj_idx = np.stack([rng.choice(np.delete(np.arange(M), s), A, replace=False) for s in range(M)]).astype(np.int32)
    adj_idx[rng.random((M, A)) < 0.2] = -1
    knn_idx[10, 0], adj_idx[10, 1], knn_idx[11, 3], adj_idx[11, 0] = 11, 11, 10, 10      # present in both lists, both directions
    adj_idx[12, 0], adj_idx[3, 0] = 3, 12                                                # a NaN row as a neighbour, and as the owner
    return feat, knn_idx, knn_sim, adj_idx


def check_lists(feat, knn_idx, knn_sim, adj_idx, got_idx, got_sim):
    ref_idx, ref_sim = merge_lists_host(feat, knn_idx, knn_sim, adj_idx)
    got_idx, got_sim = got_idx.cpu().numpy(), got_sim.cpu().numpy()
    k = 0 if knn_idx is None else knn_idx.shape[1]
    assert np.array_equal(got_idx, ref_idx)
    if k:
        assert got_sim[:, :k].tobytes() == np.asarray(knn_sim, np.float32).tobytes()      # copied
    f = np.asarray(feat, np.float32).astype(np.float64)
    M = f.shape[0]
    worst = 0.0
    for s in range(M):
        for a in range(k, got_idx.shape[1]):
            t = int(ref_idx[s, a])
            if t < 0:
                assert got_sim[s, a] == -np.inf
                continue
            prod = f[s] * f[t]
            if np.isnan(prod).any():
                assert np.isnan(got_sim[s, a]) and np.isnan(ref_sim[s, a])
                continue
            bound = 1.001 * 1024 * 2.0 ** -24 * np.abs(prod).sum()
            err = abs(float(got_sim[s, a]) - prod.sum())
            worst = max(worst, err / bound)
            assert err <= bound, (s, a, err, bound)
    return worst


def test_the_lists_are_the_definition():
    feat, knn_idx, knn_sim, adj_idx = lists_case()
    idx, sim = merge_lists(_dev(feat), _dev(knn_idx), _dev(knn_sim), _dev(adj_idx))
    worst = check_lists(feat, knn_idx, knn_sim, adj_idx, idx, sim)
    print("lists: worst error / bound = %.3g" % worst)
    got = idx.cpu().numpy()
    assert got[10, 5 + 1] == -1 and got[11, 5 + 0] == -1                             # already a kNN neighbour, in both directions
    assert got[12, 5] == 3 and bool(torch.isnan(sim[12, 5])) and got[3, 5] == 12 and bool(torch.isnan(sim[3, 5]))
    idx0, sim0 = merge_lists(_dev(feat), None, None, _dev(adj_idx))                  # k = 0
    check_lists(feat, None, None, adj_idx, idx0, sim0)
    idxA, simA = merge_lists(_dev(feat), _dev(knn_idx), _dev(knn_sim), None)         # A = 0
    assert np.array_equal(idxA.cpu().numpy(), knn_idx) and simA.cpu().numpy().tobytes() == knn_sim.tobytes()
    big = lists_case(M=33, k=16, A=16, seed=3)                                       # k + A = 32, the longest list
    check_lists(*big, *merge_lists(*(_dev(a) for a in big)))
    one = (feat[:1], None, None, np.array([[-1, 0]], np.int32))                      # M = 1: itself as an adjacent region
    check_lists(*one, *merge_lists(_dev(one[0]), None, None, _dev(one[3])))


def _raw_calls(lib, st, ids, rows, cols, M, A, X, feat, knn_idx, knn_sim, fill):
    """the three entry points over buffers filled with ``fill``, one guard element behind every output"""
    n, B, k = rows * cols, X.shape[1], knn_idx.shape[1]
    nbytes = lib.cmlpl_rg_workspace_bytes(rows, cols, M, A)
    ws = torch.full((nbytes + 16,), fill, dtype=torch.uint8, device=DEV)
    def new(count, dt):
        return torch.full(((count + 1) * torch.tensor([], dtype=dt).element_size(),), fill, dtype=torch.uint8, device=DEV).view(dt)
    mean, cnt, S = new(M * B, torch.float32), new(M, torch.int64), new(M * B, torch.int64)
    adj_idx, adj_len, deg, boundary = (new(c, torch.int32) for c in (M * A, M * A, M, M))
    nbr_idx, nbr_sim = new(M * (k + A), torch.int32), new(M * (k + A), torch.float32)
    guards = [t[-1:].clone() for t in (mean, cnt, S, adj_idx, adj_len, deg, boundary, nbr_idx, nbr_sim)]
    assert lib.cmlpl_rg_pool(ids.data_ptr(), rows, cols, M, X.data_ptr(), X.stride(0), B, mean.data_ptr(), cnt.data_ptr(),
                             S.data_ptr(), ws.data_ptr(), nbytes, st) == 0
    assert lib.cmlpl_rg_adjacency(ids.data_ptr(), rows, cols, M, A, adj_idx.data_ptr(), adj_len.data_ptr(), deg.data_ptr(),
                                  boundary.data_ptr(), ws.data_ptr(), nbytes, st) == 0
    assert lib.cmlpl_rg_lists(feat.data_ptr(), M, knn_idx.data_ptr(), knn_sim.data_ptr(), k, adj_idx.data_ptr(), A,
                              nbr_idx.data_ptr(), nbr_sim.data_ptr(), st) == 0
    torch.cuda.synchronize()
    outs = (mean, cnt, S, adj_idx, adj_len, deg, boundary, nbr_idx, nbr_sim)
    for t, g in zip(outs, guards):                                                   # nothing past the ends
        assert t[-1:].cpu().numpy().tobytes() == g.cpu().numpy().tobytes()
    assert (ws[nbytes:] == fill).all()
    return [t[:-1].cpu().numpy() for t in outs]


def test_two_runs_over_different_previous_contents_give_the_same_bytes():
    from cmlpl_amd import _lib
    lib, st = _lib.load(), _stream()
    rows, cols, A, B, k = 61, 47, 4, 103, 3
    for name in ("smoothed_components", "hub", "voids"):
        ids, M = region_map(name, rows, cols)
        n = rows * cols
        assert lib.cmlpl_rg_workspace_bytes(rows, cols, M, A) == 16 + 4 * (3 * M + 1 + (M + 1023) // 1024 + 2 + 33 * n)
        X = pool_input(n, B)
        rng = np.random.default_rng(M)
        feat = rng.standard_normal((M, 1024)).astype(np.float32)
        knn_idx = rng.integers(-1, M, (M, k)).astype(np.int32)
        knn_sim = rng.random((M, k)).astype(np.float32)
        args = [_dev(a) for a in (ids, X, feat, knn_idx, knn_sim)]
        runs = [_raw_calls(lib, st, args[0], rows, cols, M, A, *args[1:], fill) for fill in (0x00, 0xFF, 0x7F)]
        for other in runs[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(other, runs[0])), name
        ref_p, ref_a = pool_host(ids, M, X), adjacency_host(ids, M, rows, cols, A)
        mean, cnt, S, adj_idx, adj_len, deg, boundary, nbr_idx, nbr_sim = runs[0]
        assert mean.tobytes() == ref_p["mean"].tobytes() and np.array_equal(cnt, ref_p["cnt"]) and np.array_equal(S, ref_p["S"].ravel())
        assert np.array_equal(adj_idx.reshape(M, A), ref_a["adj_idx"]) and np.array_equal(adj_len.reshape(M, A), ref_a["adj_len"])
        assert np.array_equal(deg, ref_a["deg"]) and np.array_equal(boundary, ref_a["boundary"])
        assert np.array_equal(nbr_idx.reshape(M, k + A), merge_lists_host(feat, knn_idx, knn_sim, ref_a["adj_idx"])[0])


def test_a_call_captured_in_a_graph_replays_the_eager_bytes():
    rows, cols, A = 61, 47, 8
    ids_h, M = region_map("smoothed_components", rows, cols)
    ids, X = _dev(ids_h), _dev(pool_input(rows * cols, 60))
    feat = torch.randn(M, 1024, device=DEV)

    def run():
        p, a = pool(ids, M, X, sums=True), adjacency(ids, M, rows, cols, A)
        return (p.mean, p.cnt, p.S, a.adj_idx, a.adj_len, a.deg, a.boundary, *merge_lists(feat, None, None, a.adj_idx))
    eager = run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def e2e_device():
    """the end-to-end case on the device: the member network, the superpixel vote (the plain map: the case the CPU test holds
    to the comparison's own conditions)"""
    from cmlpl_amd.models import BaseNet2
    from cmlpl_amd.superpixel import Superpixel, superpixel_probs
    c = e2e_case()
    shape = c["shape"]
    net = BaseNet2(num_features=shape[3], dropout=0.8, num_classes=shape[4], in_channels=shape[0], window=shape[1]).to(DEV)
    net.load_state_dict(c["params"])
    net.eval()
    vote = superpixel_probs(_dev(c["p"]), _dev(c["cube"]), Superpixel(E2E["step"], guide=E2E["G"]))
    return net, vote, _dev(c["spectra"])


@pytest.mark.parametrize("cfg", [RegionGraph(), RegionGraph(k=4, adj=4, alpha=0.9, iters=50)], ids=["default", "alpha0.9"])
def test_end_to_end_against_the_host_on_the_devices_lists(cfg):
    rows, cols = E2E["rows"], E2E["cols"]
    net, vote, spectra = e2e_device()
    ids, M = vote.segments.seg, vote.segments.N
    assert 100 <= M <= 1000
    rg = region_graph(ids, M, rows, cols, spectra, [net], cfg)
    out = region_propagate(rg, vote.seg_probs, cfg, conf=True, entropy=True)
    ids_h, q = ids.cpu().numpy(), vote.seg_probs.cpu().numpy()
    # the pieces in front of the lists: the pool bit for bit, the adjacency exactly, the lists by their own definition
    ref_p = pool_host(ids_h, M, e2e_case()["spectra"])
    assert rg.pooled.mean.cpu().numpy().tobytes() == ref_p["mean"].tobytes() and np.array_equal(rg.pooled.cnt.cpu().numpy(), ref_p["cnt"])
    ref_a = adjacency_host(ids_h, M, rows, cols, cfg.adj)
    assert np.array_equal(rg.adjacency.adj_idx.cpu().numpy(), ref_a["adj_idx"]) and np.array_equal(rg.adjacency.deg.cpu().numpy(), ref_a["deg"])
    lists = (rg.nbr_idx.cpu().numpy(), rg.nbr_sim.cpu().numpy())
    assert lists[0].shape == (M, cfg.k + cfg.adj)
    check_lists(rg.feat.cpu().numpy(), lists[0][:, :cfg.k], lists[1][:, :cfg.k], ref_a["adj_idx"], rg.nbr_idx, rg.nbr_sim)
    # the host's definition on the device's lists
    h64 = region_graph_host(ids_h, M, rows, cols, None, q, cfg, lists=lists)
    h32 = region_graph_host(ids_h, M, rows, cols, None, q, cfg, lists=lists, dtype=np.float32)
    g, r = rg.graph, out.regions
    got = dict(cinv=g.cinv.cpu().numpy(), fwd_coef=g.fwd_coef.cpu().numpy(), rev_coef=g.rev_coef[:g.edges()].cpu().numpy(),
               F=r.F.cpu().numpy(), probs=r.probs.cpu().numpy(), conf=r.conf.cpu().numpy(), entropy=r.entropy.cpu().numpy(),
               residual=float(r.residual.cpu()[0]), labels=r.labels.cpu().numpy())
    U.compare("region graph %s" % (cfg,), got, h64["lp"], h32["lp"])
    assert np.array_equal(out.Y.cpu().numpy(), h64["Y"])
    # the pixel outputs are the gather of the region outputs, bit for bit; void and unreached pixels are -1 / NaN
    inside = (ids_h >= 0) & (ids_h < M)
    at = np.where(inside, ids_h, 0)
    assert np.array_equal(out.labels.cpu().numpy(), np.where(inside, got["labels"][at], -1))
    for name, per_pixel in (("probs", out.probs), ("conf", out.conf), ("entropy", out.entropy)):
        want = got[name][at].copy()
        want[~inside] = np.nan
        assert per_pixel.cpu().numpy().tobytes() == want.astype(np.float32).tobytes(), name
    oa = lambda lab: float((lab == e2e_case()["Y"]).mean())
    print("OA vote %.4f, region graph %.4f" % (oa(vote.labels.cpu().numpy()), oa(out.labels.cpu().numpy())))


def test_voids_unreached_regions_alpha_zero_and_seeds():
    rows, cols, K = E2E["rows"], E2E["cols"], E2E["K"]
    net, vote, spectra = e2e_device()
    from cmlpl_amd.superpixel import region_vote, region_vote_host
    ids_h = vote.segments.seg.cpu().numpy().copy()
    M = vote.segments.N
    ids_h[ids_h == 7] = -1                                                           # region 7 becomes empty, its pixels void
    ids_h[ids_h == 9] = M + 3                                                        # and region 9's an id past M
    ids = _dev(ids_h)
    rv = region_vote(ids, probs=_dev(e2e_case()["p"]), N=M)
    assert bool(torch.isnan(rv.seg_probs[7]).all())
    cfg = RegionGraph(k=3, adj=3)
    rg = region_graph(ids, M, rows, cols, spectra, net, cfg)
    assert bool(torch.isnan(rg.feat[7]).all()) and int(rg.pooled.cnt[7]) == 0 and int(rg.adjacency.deg[7]) == 0
    assert not bool((rg.nbr_idx == 7).any()) and not bool((rg.nbr_idx == 9).any())   # nobody takes an empty region as a neighbour
    out = region_propagate(rg, rv.seg_probs, cfg, conf=True, entropy=True)
    assert int(out.regions.labels[7]) == -1 and bool((out.Y[7] == 0).all())          # a NaN row became a zero row: unreached
    void = torch.from_numpy((ids_h < 0) | (ids_h >= M)).to(DEV)
    assert bool(void.any()) and bool((out.labels[void] == -1).all())
    assert bool(torch.isnan(out.probs[void]).all()) and bool(torch.isnan(out.conf[void]).all()) and bool(torch.isnan(out.entropy[void]).all())
    assert bool((out.labels[~void] >= 0).all()) and not bool(torch.isnan(out.probs[~void]).any())
    zero = region_propagate(rg, rv.seg_probs, RegionGraph(k=3, adj=3, alpha=0.0))    # alpha = 0 returns the vote's labels
    assert torch.equal(zero.labels, rv.labels)
    # seeds REPLACE the Y row of every region that holds one with its normalised class histogram
    Y = e2e_case()["Y"]
    pix = np.arange(0, rows * cols, 11)
    seeded = region_propagate(rg, rv.seg_probs, cfg, seeds=(pix, Y[pix]))
    tm = np.full(rows * cols, -1, np.int64)
    tm[pix] = Y[pix]
    hist = region_vote_host(ids_h, M, K, labels=tm)
    has = hist["cnt"] > 0
    assert has.any()
    assert np.array_equal(seeded.Y.cpu().numpy()[has], hist["q"][has]) and torch.equal(seeded.Y[_dev(~has)], out.Y[_dev(~has)])
    host = region_graph_host(ids_h, M, rows, cols, None, rv.seg_probs.cpu().numpy(), cfg, seeds=(pix, Y[pix]),
                             lists=(rg.nbr_idx.cpu().numpy(), rg.nbr_sim.cpu().numpy()))
    assert np.array_equal(seeded.Y.cpu().numpy(), host["Y"])


def test_the_library_refuses_what_it_cannot_take():
    from cmlpl_amd import _lib
    lib, st = _lib.load(), _stream()
    rows, cols, M, A, B, k = 12, 9, 7, 3, 5, 2
    n = rows * cols
    wsb = lib.cmlpl_rg_workspace_bytes
    assert wsb(0, 5, M, A) == 0 and wsb(5, -1, M, A) == 0 and wsb(rows, cols, 0, A) == 0 and wsb(rows, cols, M, 17) == 0
    assert wsb(rows, cols, M, -1) == 0 and wsb(16384, 8193, M, A) == 0 and wsb(rows, cols, 2 ** 27 + 1, A) == 0
    need = wsb(rows, cols, M, A)
    assert need == 16 + 4 * (3 * M + 1 + 1 + 2 + 33 * n) and wsb(16384, 8192, M, A) > 0
    ids = torch.randint(0, M, (n,), dtype=torch.int32, device=DEV)
    X = torch.randn(n, B, device=DEV)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    f32 = lambda count: torch.full((count,), 7.0, device=DEV)
    i32 = lambda count: torch.full((count,), -7, dtype=torch.int32, device=DEV)
    mean, cnt, S = f32(M * B), torch.full((M,), -7, dtype=torch.int64, device=DEV), torch.full((M * B,), -7, dtype=torch.int64, device=DEV)
    okp = dict(ids=ids.data_ptr(), rows=rows, cols=cols, M=M, X=X.data_ptr(), stride=B, B=B, mean=mean.data_ptr(), cnt=cnt.data_ptr(),
               S=S.data_ptr(), ws=ws.data_ptr(), nb=need)
    poolc = lambda a: lib.cmlpl_rg_pool(a["ids"], a["rows"], a["cols"], a["M"], a["X"], a["stride"], a["B"], a["mean"], a["cnt"], a["S"],
                                        a["ws"], a["nb"], st)
    for change in (dict(rows=0), dict(cols=0), dict(rows=16384, cols=8193), dict(M=0), dict(M=2 ** 27 + 1), dict(B=0), dict(B=1025),
                   dict(stride=B - 1), dict(ids=None), dict(X=None), dict(mean=None), dict(cnt=None), dict(ws=None),
                   dict(ids=ids.data_ptr() + 2), dict(X=X.data_ptr() + 1), dict(mean=mean.data_ptr() + 2), dict(cnt=cnt.data_ptr() + 4),
                   dict(S=S.data_ptr() + 4), dict(ws=ws.data_ptr() + 1)):
        assert poolc(dict(okp, **change)) == -1, change
    assert poolc(dict(okp, nb=need - 1)) == -3
    adj_idx, adj_len, deg, boundary = i32(M * A), i32(M * A), i32(M), i32(M)
    oka = dict(ids=ids.data_ptr(), rows=rows, cols=cols, M=M, A=A, idx=adj_idx.data_ptr(), len=adj_len.data_ptr(), deg=deg.data_ptr(),
               bnd=boundary.data_ptr(), ws=ws.data_ptr(), nb=need)
    adjc = lambda a: lib.cmlpl_rg_adjacency(a["ids"], a["rows"], a["cols"], a["M"], a["A"], a["idx"], a["len"], a["deg"], a["bnd"],
                                            a["ws"], a["nb"], st)
    for change in (dict(rows=0), dict(cols=-2), dict(rows=16384, cols=8193), dict(M=0), dict(A=-1), dict(A=17), dict(ids=None),
                   dict(idx=None), dict(len=None), dict(deg=None), dict(bnd=None), dict(ws=None), dict(ids=ids.data_ptr() + 1),
                   dict(idx=adj_idx.data_ptr() + 2), dict(len=adj_len.data_ptr() + 3), dict(deg=deg.data_ptr() + 2),
                   dict(bnd=boundary.data_ptr() + 1), dict(ws=ws.data_ptr() + 2)):
        assert adjc(dict(oka, **change)) == -1, change
    assert adjc(dict(oka, nb=need - 1)) == -3
    feat = torch.randn(M + 1, 1024, device=DEV)
    knn_idx, knn_sim = torch.zeros(M, k, dtype=torch.int32, device=DEV), torch.zeros(M, k, device=DEV)
    aidx = torch.full((M, A), -1, dtype=torch.int32, device=DEV)
    nbr_idx, nbr_sim = i32(M * 32), f32(M * 32)
    okl = dict(feat=feat.data_ptr(), M=M, ki=knn_idx.data_ptr(), ks=knn_sim.data_ptr(), k=k, ai=aidx.data_ptr(), A=A,
               ni=nbr_idx.data_ptr(), ns=nbr_sim.data_ptr())
    listc = lambda a: lib.cmlpl_rg_lists(a["feat"], a["M"], a["ki"], a["ks"], a["k"], a["ai"], a["A"], a["ni"], a["ns"], st)
    for change in (dict(M=0), dict(k=-1), dict(A=-1), dict(A=17), dict(k=0, A=0), dict(k=30), dict(k=17, A=16), dict(feat=None),
                   dict(ki=None), dict(ks=None), dict(ai=None), dict(ni=None), dict(ns=None), dict(feat=feat.data_ptr() + 4),
                   dict(ki=knn_idx.data_ptr() + 2), dict(ks=knn_sim.data_ptr() + 1), dict(ai=aidx.data_ptr() + 2),
                   dict(ni=nbr_idx.data_ptr() + 1), dict(ns=nbr_sim.data_ptr() + 2)):
        assert listc(dict(okl, **change)) == -1, change
    torch.cuda.synchronize()
    for t in (cnt, S, adj_idx, adj_len, deg, boundary, nbr_idx):                      # nothing was launched
        assert (t == -7).all()
    assert (mean == 7.0).all() and (nbr_sim == 7.0).all()
    assert poolc(okp) == 0 and poolc(dict(okp, S=None, ws=ws.data_ptr() + 4)) == 0
    assert adjc(oka) == 0 and adjc(dict(oka, A=0, idx=None, len=None)) == 0
    assert listc(okl) == 0 and listc(dict(okl, k=0, ki=None, ks=None)) == 0 and listc(dict(okl, A=0, ai=None)) == 0
    torch.cuda.synchronize()
    assert (cnt >= 0).all() and (deg >= 0).all()
    # and the Python layer, before any launch
    for bad in (lambda: pool(ids, M, X.double()), lambda: pool(ids, 0, X), lambda: pool(ids[:-1], M, X),
                lambda: adjacency(ids, M, rows, cols, 17), lambda: adjacency(ids, M, rows, cols + 1, 2),
                lambda: merge_lists(feat[:M], None, None, None), lambda: merge_lists(feat[:M], knn_idx, None, aidx),
                lambda: region_graph(ids, M, rows, cols, X, [None], RegionGraph(k=20, adj=16)),
                lambda: region_graph(ids, M, rows, cols, X, [None], RegionGraph(net=1))):
        with pytest.raises(ValueError):
            bad()
