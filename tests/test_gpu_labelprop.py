"""GPU: label propagation (csrc/labelprop.hip) against the definition restated in numpy (cmlpl_amd.labelprop.labelprop_host).

Every quantity is held to tol = 8 max|host fp32 - host fp64| of the host's fp64, per quantity (the pattern of
tests/test_gpu_smooth.py); labels to the host's on every SURE row -- a row whose fp64 top-2 gap in F exceeds 2 tol_F: a device
row within tol_F cannot order the two differently.  The inputs are chosen so that, for the host ALONE, at least 99 % of the rows
are sure and no fp64 row sum is below 1e-4 (tests/lp_util.compare asserts both before it looks at the device)."""
import numpy as np
import pytest
import torch

from cmlpl_amd.labelprop import (LabelProp, build_graph, graph_bytes, knn_graph, label_propagation, labelprop_host,
                                 one_hot_seeds, propagate)
from tests import lp_util as U
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

#        n,   k,  K, alpha, gamma, iters, seed, dense Y
CASES = [(1500, 5, 1, 0.9, 3, 20, 0, False),          # G = 1; the hub's in-degree 1,499 crosses 64, 256 and 1,024
         (1500, 5, 9, 0.9, 3, 20, 0, False),          # G = 16
         (1500, 5, 17, 0.9, 3, 20, 0, False),         # G = 32
         (1500, 5, 64, 0.9, 3, 20, 0, False),         # G = 64
         (1500, 5, 2, 0.9, 3, 20, 0, False),          # G = 2
         (1500, 5, 3, 0.9, 3, 20, 0, False),          # G = 4
         (1500, 5, 5, 0.9, 3, 20, 0, False),          # G = 8
         (300, 32, 9, 0.5, 3, 10, 0, False),          # the longest lists
         (1500, 5, 9, 0.9, 1, 20, 0, False),
         (1500, 5, 17, 0.9, 8, 20, 0, False),         # (K = 17, 51 seeds: with K = 9 the smallest fp64 row sum is 9.7e-5, under
                                                      #  the cap for the host alone -- weights s^8 carry little)
         (1500, 5, 9, 0.9, 3, 20, 0, True),
         (2600, 5, 9, 0.9, 3, 10, 0, False)]          # in-degree 2,599 > 2,048: the segment that is re-found by the compaction scan


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                # (a copy: the shared inputs are read-only)


def _run(idx, sim, Y, alpha, gamma, iters, **kw):
    g = build_graph(_dev(idx), _dev(sim), gamma)
    return g, propagate(g, _dev(Y), alpha, iters, **kw)


def _got(g, res):
    E = g.edges()
    return dict(cinv=g.cinv.cpu().numpy(), fwd_coef=g.fwd_coef.cpu().numpy(), rev_coef=g.rev_coef[:E].cpu().numpy(),
                F=res.F.cpu().numpy(), probs=res.probs.cpu().numpy(), conf=res.conf.cpu().numpy(),
                entropy=res.entropy.cpu().numpy(), residual=float(res.residual.cpu()[0]), labels=res.labels.cpu().numpy())


@pytest.mark.parametrize("n,k,K,alpha,gamma,iters,seed,dense", CASES)
def test_kernels_against_the_host(n, k, K, alpha, gamma, iters, seed, dense):
    idx, sim, Y = U.hub_graph(n, k, K, seed, dense)
    h64, h32 = U.host_pair(n, k, K, alpha, gamma, iters, seed, dense)
    g, res = _run(idx, sim, Y, alpha, gamma, iters, conf=True, entropy=True, residual=True)
    E = g.edges()
    assert np.array_equal(g.rev_ptr.cpu().numpy(), h64.rev_ptr) and np.array_equal(g.rev_src[:E].cpu().numpy(), h64.rev_src)
    assert bool((g.rev_src[E:] == -1).all()) and bool((g.rev_coef[E:] == 0).all())
    assert g.max_in_degree() == n - 1 == int(np.diff(h64.rev_ptr).max())
    assert np.array_equal(g.fwd_dst.cpu().numpy(), np.where((idx >= 0) & (idx != np.arange(n)[:, None]), idx, -1))
    src, k_of = g.rev_edge[:E].cpu().numpy() // k, g.rev_edge[:E].cpu().numpy() % k
    assert np.array_equal(src, h64.rev_src) and np.array_equal(idx[src, k_of], np.repeat(np.arange(n), np.diff(h64.rev_ptr)))
    U.compare("n=%d k=%d K=%d gamma=%d%s" % (n, k, K, gamma, " dense" if dense else ""), _got(g, res), h64, h32)
    assert bool((res.labels >= 0).all()) == bool((h64.labels >= 0).all())


def test_two_runs_give_the_same_bytes_graph_included():
    idx, sim, Y = U.hub_graph(1500, 5, 9)
    kw = dict(conf=True, entropy=True, residual=True)
    torch.cuda.empty_cache()
    g1, r1 = _run(idx, sim, Y, 0.9, 3, 20, **kw)
    junk = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=DEV)             # (other bytes under the next buffers)
    del junk
    g2, r2 = _run(idx, sim, Y, 0.9, 3, 20, **kw)
    assert torch.equal(g1.buf, g2.buf)
    for a, b in zip(r1, r2):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_ten_and_ten_iterations_are_twenty():
    idx, sim, Y = U.hub_graph(1500, 5, 9)
    g = build_graph(_dev(idx), _dev(sim), 3)
    Yd = _dev(Y)
    kw = dict(conf=True, entropy=True, residual=True)
    a = propagate(g, Yd, 0.9, 10)
    b, c = propagate(g, Yd, 0.9, 10, F0=a.F, **kw), propagate(g, Yd, 0.9, 20, **kw)
    for x, y in zip(b, c):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    odd = propagate(g, Yd, 0.9, 7, F0=propagate(g, Yd, 0.9, 13).F, **kw)           # (an odd leg ends in the other buffer)
    assert odd.F.cpu().numpy().tobytes() == c.F.cpu().numpy().tobytes()


@pytest.mark.parametrize("K,dense", [(9, False), (5, True)])
def test_alpha_zero_returns_the_bytes_of_y(K, dense):
    idx, sim, Y = U.hub_graph(1500, 5, K, 0, dense)
    for iters in (1, 4):
        _, res = _run(idx, sim, Y, 0.0, 3, iters, residual=True)
        assert res.F.cpu().numpy().tobytes() == Y.tobytes()
    assert float(res.residual.cpu()[0]) == 0.0


def test_null_outputs_change_nothing_else_and_y_is_left_alone():
    idx, sim, Y = U.hub_graph(1500, 5, 9)
    g = build_graph(_dev(idx), _dev(sim), 3)
    Yd = _dev(Y)
    full = propagate(g, Yd, 0.9, 20, conf=True, entropy=True, residual=True)
    bare = propagate(g, Yd, 0.9, 20, probs=False)
    assert bare.probs is None and bare.conf is None and bare.entropy is None and bare.residual is None
    assert torch.equal(bare.F, full.F) and torch.equal(bare.labels, full.labels)
    for name in ("probs", "conf", "entropy", "residual"):
        one = propagate(g, Yd, 0.9, 20, **{**dict(probs=False), name: True})
        assert getattr(one, name).cpu().numpy().tobytes() == getattr(full, name).cpu().numpy().tobytes()
        assert torch.equal(one.F, full.F) and torch.equal(one.labels, full.labels)
    assert Yd.cpu().numpy().tobytes() == Y.tobytes()
    # the C entry point with every optional output NULL: F alone
    from cmlpl_amd import _lib
    F, tmp = torch.empty_like(Yd), torch.empty_like(Yd)
    rc = _lib.load().cmlpl_lp_propagate(g.buf.data_ptr(), g.n, g.k, Yd.data_ptr(), 9, 0.9, 20, None, F.data_ptr(), tmp.data_ptr(),
                                        None, None, None, None, None, None)
    assert rc == 0 and torch.equal(F, full.F)


def test_one_hot_seeds():
    lab = torch.tensor([0, 3, -1, 4, 2, 99], dtype=torch.int64, device=DEV)
    Y = one_hot_seeds(lab, 4).cpu().numpy()
    assert Y.dtype == np.float32 and np.array_equal(Y, U.one_hot(lab.cpu().numpy(), 4))


def test_end_to_end_on_the_arcs():
    n_per, dphi, k = U.ARC_CASES[0]
    X, truth, seeds = U.arcs(n_per, dphi)
    feat = _dev(X)
    cfg = LabelProp(k=k, alpha=U.ARC_ALPHA, gamma=U.ARC_GAMMA, iters=U.ARC_ITERS)
    res = label_propagation(feat, _dev(seeds), 9, cfg, conf=True, entropy=True, residual=True)
    idx, sim = knn_graph(feat, k)
    g = build_graph(idx, sim, cfg.gamma)
    hosts = [labelprop_host(idx.cpu().numpy(), sim.cpu().numpy(), U.one_hot(seeds, 9), cfg.alpha, cfg.gamma, cfg.iters, dtype=dt)
             for dt in (np.float64, np.float32)]
    assert np.array_equal(g.rev_ptr.cpu().numpy(), hosts[0].rev_ptr)
    assert np.array_equal(g.rev_src[:g.edges()].cpu().numpy(), hosts[0].rev_src)
    U.compare("arcs n=%d k=%d" % (len(truth), k), _got(g, res), *hosts)
    labels = res.labels.cpu().numpy()
    near, got = U.nearest_seed_accuracy(X, truth, seeds), float((labels == truth).mean())
    print("nearest seed %.3f, propagated %.3f" % (near, got))
    assert (labels >= 0).all()
    assert got >= near + 0.10


def test_the_library_refuses_what_it_cannot_take():
    from cmlpl_amd import _lib
    lib = _lib.load()
    n, k, K = 40, 4, 3
    idx, sim, Y = (_dev(a) for a in U.hub_graph(n, k, K))
    assert [lib.cmlpl_lp_graph_bytes(*a) for a in ((0, 4), (4, 0), (4, 33), (1 << 27, 16), (-1, 4))] == [0] * 5
    assert lib.cmlpl_lp_graph_bytes(n, k) == 4 * (3 * n + 1 + 5 * n * k) == graph_bytes(n, k)
    assert lib.cmlpl_lp_graph_bytes((1 << 27) - 1, 16) > 0
    buf = torch.empty(graph_bytes(n, k), dtype=torch.uint8, device=DEV)
    ok = dict(idx=idx.data_ptr(), sim=sim.data_ptr(), n=n, k=k, gamma=3, buf=buf.data_ptr(), size=buf.numel())
    graph = lambda **kw: (lambda a: lib.cmlpl_lp_graph(a["idx"], a["sim"], a["n"], a["k"], a["gamma"], a["buf"], a["size"], None))({**ok, **kw})
    for bad in (dict(idx=None), dict(sim=None), dict(buf=None), dict(n=0), dict(k=0), dict(k=33), dict(gamma=0), dict(gamma=9),
                dict(idx=idx.data_ptr() + 2), dict(sim=sim.data_ptr() + 1), dict(buf=buf.data_ptr() + 2), dict(n=1 << 27, k=16)):
        assert graph(**bad) == -1, bad
    assert graph(size=buf.numel() - 1) == -3
    assert graph() == 0
    F, tmp, F0 = (torch.empty(n, K, device=DEV) for _ in range(3))
    out = dict(probs=None, labels=None, conf=None, entropy=None, residual=None)
    okp = dict(buf=buf.data_ptr(), n=n, k=k, Y=Y.data_ptr(), K=K, alpha=0.5, iters=2, F0=None, F=F.data_ptr(), tmp=tmp.data_ptr(), **out)
    prop = lambda **kw: (lambda a: lib.cmlpl_lp_propagate(a["buf"], a["n"], a["k"], a["Y"], a["K"], a["alpha"], a["iters"], a["F0"],
                                                          a["F"], a["tmp"], a["probs"], a["labels"], a["conf"], a["entropy"],
                                                          a["residual"], None))({**okp, **kw})
    lab8 = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    for bad in (dict(buf=None), dict(Y=None), dict(F=None), dict(tmp=None), dict(n=0), dict(k=0), dict(k=33), dict(K=0), dict(K=65),
                dict(alpha=1.0), dict(alpha=-0.5), dict(alpha=float("nan")), dict(iters=0), dict(iters=10001),
                dict(tmp=F.data_ptr()), dict(F=Y.data_ptr()), dict(tmp=Y.data_ptr()), dict(F0=F.data_ptr()), dict(F0=tmp.data_ptr()),
                dict(Y=Y.data_ptr() + 2), dict(probs=F0.data_ptr() + 1), dict(labels=lab8.data_ptr() + 4), dict(residual=F0.data_ptr() + 2)):
        assert prop(**bad) == -1, bad
    assert prop() == 0 and prop(F0=F0.fill_(0.5).data_ptr()) == 0 and prop(F0=Y.data_ptr()) == 0
    torch.cuda.synchronize()
    for bad in (dict(alpha=1.0), dict(iters=0)):
        with pytest.raises(ValueError):
            propagate(build_graph(idx, sim), Y, **{**dict(alpha=0.5, iters=1), **bad})
    with pytest.raises(ValueError):
        build_graph(idx, sim, gamma=9)
    with pytest.raises(ValueError):
        build_graph(idx.to(torch.int64), sim)
