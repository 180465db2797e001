"""GPU: the superpixel and region-vote kernels (csrc/superpixel.hip) against the definitions restated in numpy
(cmlpl_amd.superpixel.segment_host / region_vote_host).  The definitions fix every rounding and every sum is an integer, so
the map, the counts, the centres, P, cnt, q, the labels and the confidence are held EXACTLY: every int, every float's bits.

The entropy is the one output that goes through logf, which is not libm's on the device.  It is held by the allowance rule
of tests/test_gpu_ensemble.py: the yardstick is the error of the SAME arithmetic in fp32 by numpy on the CPU against fp64 on
the same q, and the device is allowed 8 x that per case -- a case being one (K, source) with all its maps."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmlpl_amd.superpixel import (Superpixel, asa, region_vote, region_vote_host, segment, segment_host, superpixel_probs)
from tests.gpu_util import DEV
from tests.test_smooth_host import case

pytestmark = pytest.mark.gpu

# (rows, cols, cube channels, G, S): the edge shapes, the builder's cases, steps that do not divide the tile, S = 2 with
# more than one tile across (the widest block of candidate centres in LDS), and both sides of the step (12) from which a
# whole workgroup gathers a segment
SHAPES = [(1, 1, 5, 3, 4), (3, 50, 5, 3, 8), (50, 3, 5, 0, 4), (9, 9, 12, 8, 2), (17, 13, 5, 3, 64), (37, 29, 7, 3, 4),
          (61, 47, 7, 3, 6), (37, 29, 7, 3, 5), (40, 23, 7, 3, 4), (20, 70, 6, 2, 2), (33, 65, 4, 1, 3),
          (45, 52, 6, 3, 11), (45, 52, 6, 3, 12), (50, 70, 5, 3, 16), (70, 90, 9, 8, 33)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _device_map(cube, S, m, T, G):
    r = segment(torch.from_numpy(cube).to(DEV), Superpixel(S, m, T, G))
    torch.cuda.synchronize()
    assert r.seg.dtype == torch.int32 and r.counts.dtype == torch.int32 and r.centres.dtype == torch.float32
    return r, dict(seg=r.seg.cpu().numpy(), centres=r.centres.cpu().numpy(), counts=r.counts.cpu().numpy(), ny=r.ny, nx=r.nx)


def _same_map(got, ref, tag):
    assert (got["ny"], got["nx"]) == (ref["ny"], ref["nx"]), tag
    assert got["seg"].shape == ref["seg"].shape and got["centres"].shape == ref["centres"].shape, tag
    bad = int((got["seg"] != ref["seg"]).sum())
    assert bad == 0, "%s: %d pixels labelled differently" % (tag, bad)
    assert np.array_equal(got["counts"], ref["counts"]), tag
    assert np.array_equal(_bits(got["centres"]), _bits(ref["centres"])), tag


@pytest.mark.parametrize("T", [1, 4, 10])
@pytest.mark.parametrize("rows,cols,Cc,G,S", SHAPES)
def test_the_map_is_the_definitions(rows, cols, Cc, G, S, T):
    _, cube, _ = case(rows, cols, 4, G, 1, channels=Cc)
    assert Cc > G                                               # the stride of a pixel is not its guide
    _, got = _device_map(cube, S, 1.0, T, G)
    _same_map(got, segment_host(cube, S, 1.0, T, G), "%d x %d G %d S %d T %d" % (rows, cols, G, S, T))


@pytest.mark.parametrize("m", [0.25, 3.0])
def test_other_compactness(m):
    _, cube, _ = case(37, 29, 4, 3, 2, channels=6)
    _, got = _device_map(cube, 5, m, 10, 3)
    _same_map(got, segment_host(cube, 5, m, 10, 3), "m %g" % m)


def test_irregular_pixels():
    _, cube, _ = case(24, 20, 5, 3, 2, channels=6)
    cube[5, 6, 1], cube[7, 7, 0], cube[0, 0, 2], cube[9, 9, 4] = np.nan, 3e7, -np.inf, np.nan
    for T in (1, 10):
        _, got = _device_map(cube, 4, 1.0, T, 3)
        _same_map(got, segment_host(cube, 4, 1.0, T, 3), "irregular T %d" % T)
        assert np.isfinite(got["centres"]).all() and got["counts"].sum() == 24 * 20 - 3
        for y, x in ((5, 6), (7, 7), (0, 0)):
            assert got["seg"][y * 20 + x] == (y // 4) * got["nx"] + x // 4
    cube[2, 2, 0] = np.nan                                      # the centre pixel of cell (0, 0): its first centre has a zero guide
    for T in (1, 4):
        _, got = _device_map(cube, 4, 1.0, T, 3)
        _same_map(got, segment_host(cube, 4, 1.0, T, 3), "irregular centre T %d" % T)


def test_two_runs_give_the_same_bytes_whatever_the_workspace_held():
    from cmlpl_amd import _lib
    lib = _lib.load()
    rows, cols, Cc, G, S, T = 61, 47, 7, 3, 6, 10
    _, cube, _ = case(rows, cols, 4, G, 1, channels=Cc)
    ref = segment_host(cube, S, 1.0, T, G)
    ct = torch.from_numpy(cube).to(DEV)
    N, n = ref["ny"] * ref["nx"], rows * cols
    nbytes = lib.cmlpl_sp_workspace_bytes(rows, cols, G, S)
    assert nbytes == 4 * (N * (2 + G) + G * n) + (n + 3) // 4 * 4
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for fill in (0, 255, 0x7f, 1):                              # (255: NaN centres and set flags; 1: every flag set)
        ws = torch.full((nbytes + 16,), fill, dtype=torch.uint8, device=DEV)
        seg = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
        cen = torch.full((N * (2 + G) + 1,), 7.0, device=DEV)
        cnt = torch.full((N + 1,), -7, dtype=torch.int32, device=DEV)
        assert lib.cmlpl_sp_segment(ct.data_ptr(), Cc, G, rows, cols, S, 1.0, T, seg.data_ptr(), cen.data_ptr(), cnt.data_ptr(),
                                    ws.data_ptr(), nbytes, st) == 0
        torch.cuda.synchronize()
        assert seg[-1] == -7 and cen[-1] == 7.0 and cnt[-1] == -7 and (ws[nbytes:] == fill).all()      # nothing past the ends
        outs.append((seg.cpu().numpy(), cen.cpu().numpy(), cnt.cpu().numpy()))
    for o in outs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o, outs[0]))
    assert np.array_equal(outs[0][0][:-1], ref["seg"]) and np.array_equal(outs[0][2][:-1], ref["counts"])
    assert np.array_equal(_bits(outs[0][1][:-1]), _bits(ref["centres"]).reshape(-1))
    # the centres and the counts are optional
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    seg = torch.empty(n, dtype=torch.int32, device=DEV)
    assert lib.cmlpl_sp_segment(ct.data_ptr(), Cc, G, rows, cols, S, 1.0, T, seg.data_ptr(), None, None, ws.data_ptr(), nbytes, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(seg.cpu().numpy(), ref["seg"])


def test_the_segmenter_can_be_captured_in_a_graph():
    _, cube, _ = case(37, 29, 4, 3, 1, channels=7)
    ct = torch.from_numpy(cube).to(DEV)
    p = torch.rand(37 * 29, 9, device=DEV)
    sp = Superpixel(4)
    eager = superpixel_probs(p, ct, sp, conf=True, entropy=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = superpixel_probs(p, ct, sp, conf=True, entropy=True)
    g.replay()
    torch.cuda.synchronize()
    for a, b in ((res.segments.seg, eager.segments.seg), (res.labels, eager.labels), (res.sums, eager.sums),
                 (res.probs, eager.probs), (res.entropy, eager.entropy)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------ the vote
def _maps(K, seed):
    """[(name, seg int32 [n], N)]: a segmenter's map, a random one with ids out of range and an empty segment, one row of the
    table for every pixel, one segment per pixel"""
    rows, cols = 37, 29
    n = rows * cols
    rng = np.random.default_rng(seed)
    _, cube, _ = case(rows, cols, 4, 3, 1)
    h = segment_host(cube, 4, 1.0, 4, 3)
    rnd = rng.integers(0, 40, n).astype(np.int32)
    rnd[rnd == 17] = 18                                         # segment 17 is empty
    rnd[[3, 500, n - 1]] = (-1, 41, 2 ** 30)                    # out of range (N = 41)
    runs = np.repeat(rng.integers(0, 41, n // 5 + 1), 5)[:n].astype(np.int32)     # runs that straddle the waves
    runs[runs == 17] = 16
    return [("segmenter", h["seg"], h["ny"] * h["nx"]), ("random", rnd, 41), ("runs", runs, 41), ("one", np.zeros(n, np.int32), 1),
            ("each", np.arange(n, dtype=np.int32), n)]


def _sources(K, n, seed):
    rng = np.random.default_rng(seed + 100)
    z = rng.standard_normal((n, K)).astype(np.float32) * 2
    e = np.exp(z - z.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).astype(np.float32)
    bad = rng.choice(n, 12, replace=False)
    for i, v in zip(bad, (np.nan, -0.5, 2.5, np.inf, -np.inf, -1e-30) * 2):
        p[i, rng.integers(0, K)] = v
    p[bad[-1]] = 2.0                                            # (2 is still valid)
    lab = rng.integers(0, K, n).astype(np.int64)
    lab[rng.choice(n, 9, replace=False)] = (-1, K, K + 5, -2 ** 40, 2 ** 40, 64, 2 ** 31, -1, K)
    return p, lab


def _entropy64(q):
    q = q.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 0.0 - np.where(q == 0, 0.0, q * np.log(np.where(q == 0, 1.0, q))).sum(1)


def _device_vote(seg, N, K, probs=None, labels=None):
    st = torch.from_numpy(seg).to(DEV)
    kw = dict(probs=torch.from_numpy(probs).to(DEV)) if probs is not None else dict(labels=torch.from_numpy(labels).to(DEV), K=K)
    r = region_vote(st, N=N, conf=True, entropy=True, **kw)
    torch.cuda.synchronize()
    assert r.labels.dtype == torch.int64 and r.sums.dtype == torch.int64 and r.seg_counts.dtype == torch.int64 and r.disagree is None
    return {k: getattr(r, k).cpu().numpy() for k in ("labels", "probs", "conf", "entropy", "seg_probs", "seg_labels", "seg_counts", "sums")}


@pytest.mark.parametrize("source", ["soft", "hard"])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 9, 16, 17, 64])            # every lane group: G = 1, 2, 4, 8, 16, 16, 32, 64
def test_the_vote_is_the_definitions(K, source):
    maps = _maps(K, K)
    p, lab = _sources(K, len(maps[0][1]), K)
    src = dict(probs=p) if source == "soft" else dict(labels=lab)
    yard, errs = 0.0, []
    for name, seg, N in maps:
        ref = region_vote_host(seg, N, K, **src)
        got = _device_vote(seg, N, K, **src)
        tag = "%s K %d %s" % (source, K, name)
        assert np.array_equal(got["sums"], ref["P"]), tag
        assert np.array_equal(got["seg_counts"], ref["cnt"]), tag
        assert np.array_equal(_bits(got["seg_probs"]), _bits(ref["q"])), tag
        assert np.array_equal(got["seg_labels"], ref["seg_labels"]), tag
        assert np.array_equal(got["labels"], ref["labels"]), tag
        assert np.array_equal(_bits(got["probs"]), _bits(ref["probs"])), tag
        assert np.array_equal(_bits(got["conf"]), _bits(ref["conf"])), tag
        voted = ref["labels"] >= 0
        assert np.isnan(got["entropy"][~voted]).all() and np.isnan(got["conf"][~voted]).all() and np.isnan(got["probs"][~voted]).all(), tag
        assert voted.any() and (ref["cnt"] == 0).any() == (name in ("random", "runs", "each")), tag
        e64 = _entropy64(ref["probs"][voted])
        yard = max(yard, float(np.abs(ref["entropy"][voted] - e64).max()))
        errs.append(float(np.abs(got["entropy"][voted] - e64).max()))
    print("%s K %d: entropy err %.2e (allowed %.2e)" % (source, K, max(errs), 8 * yard))
    assert max(errs) <= 8 * yard


def test_equal_tops_give_the_lower_index_and_an_empty_segment_votes_nothing():
    K, N = 9, 4
    seg = np.array([0, 0, 1, 1, 3, 3, 3, 7, -1], np.int32)      # segment 2 is empty
    p = np.zeros((9, K), np.float32)
    p[0, 6] = p[1, 2] = 0.5                                     # segment 0: classes 2 and 6 tie
    p[0, 0] = p[1, 0] = 0.125
    p[2, 8] = p[3, 8] = 1.0
    p[4:7, 4] = p[4:7, 5] = 0.375
    got = _device_vote(seg, N, K, probs=p)
    assert got["seg_labels"].tolist() == [2, 8, -1, 4] and got["seg_counts"].tolist() == [2, 2, 0, 3]
    assert got["labels"].tolist() == [2, 2, 8, 8, 4, 4, 4, -1, -1]
    assert np.isnan(got["seg_probs"][2]).all() and np.isnan(got["probs"][7:]).all() and np.isnan(got["entropy"][7:]).all()
    assert got["conf"][:7].tolist() == [0.25, 0.25, 1.0, 1.0, 0.375, 0.375, 0.375] and got["entropy"][2] == 0.0
    hard = _device_vote(seg, N, K, labels=np.array([5, 3, 1, 1, 2, 2, 9, 0, 0], np.int64))
    assert hard["seg_labels"].tolist() == [3, 1, -1, 2] and hard["seg_counts"].tolist() == [2, 2, 0, 2]
    assert hard["labels"].tolist() == [3, 3, 1, 1, 2, 2, 2, -1, -1]            # (the row with label 9 is repaired by its region)
    assert hard["conf"][:7].tolist() == [0.5, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0]


def test_asa_and_the_two_halves_together():
    rows, cols, K, S = 61, 47, 9, 6
    p, cube, Y = case(rows, cols, K, 3, 1, channels=7)
    ref = segment_host(cube, S, 1.0, 10, 3)
    N = ref["ny"] * ref["nx"]
    ct, pt = torch.from_numpy(cube).to(DEV), torch.from_numpy(p).to(DEV)
    test_rows = np.arange(1, rows * cols, 3)
    for vote in ("soft", "hard"):
        res = superpixel_probs(pt, ct, Superpixel(S, vote=vote), conf=True)
        torch.cuda.synchronize()
        assert res.segments.N == N and np.array_equal(res.segments.seg.cpu().numpy(), ref["seg"])
        want = region_vote_host(ref["seg"], N, K, **(dict(probs=p) if vote == "soft" else dict(labels=p.argmax(1))))
        assert np.array_equal(res.labels.cpu().numpy(), want["labels"]) and np.array_equal(_bits(res.probs.cpu().numpy()), _bits(want["probs"]))
        assert res.entropy is None and res.conf is not None
        got = asa(res.segments.seg, N, test_rows, Y[test_rows], K)
        assert got == asa(ref["seg"], N, test_rows, Y[test_rows], K) and 0.95 <= got <= 1.0
        oa = (want["labels"][test_rows] == Y[test_rows]).mean()
        print("61 x 47 S 6 %s: OA raw %.3f voted %.3f ASA %.3f" % (vote, (p.argmax(1) == Y)[test_rows].mean(), oa, got))
        assert oa <= got
    bare = superpixel_probs(pt, ct, Superpixel(S), probs_out=False)
    assert bare.probs is None and bare.conf is None and bare.labels.shape == (rows * cols,)


def test_the_library_refuses_what_it_cannot_take():
    from cmlpl_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, cols, Cc, K = 12, 9, 6, 5
    n = rows * cols
    cube = torch.rand(rows, cols, Cc, device=DEV)
    seg = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    cen = torch.full((64,), 7.0, device=DEV)
    cnt = torch.full((16,), -7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(8192, dtype=torch.uint8, device=DEV)
    inf, nan = float("inf"), float("nan")
    ok = dict(g=cube.data_ptr(), gs=Cc, G=3, rows=rows, cols=cols, S=4, m=1.0, T=3, seg=seg.data_ptr(), cen=cen.data_ptr(),
              cnt=cnt.data_ptr(), ws=ws.data_ptr(), nb=8192)
    call = lambda a: lib.cmlpl_sp_segment(a["g"], a["gs"], a["G"], a["rows"], a["cols"], a["S"], a["m"], a["T"], a["seg"], a["cen"],
                                          a["cnt"], a["ws"], a["nb"], st)
    bad = [dict(rows=0), dict(cols=0), dict(rows=65536, cols=65536), dict(G=-1), dict(G=9), dict(S=1), dict(S=65), dict(T=0), dict(T=101),
           dict(m=0.0), dict(m=-1.0), dict(m=inf), dict(m=nan), dict(m=1e-30), dict(m=1e30), dict(g=None), dict(gs=2), dict(seg=None),
           dict(ws=None), dict(nb=lib.cmlpl_sp_workspace_bytes(rows, cols, 3, 4) - 1), dict(g=cube.data_ptr() + 2),
           dict(seg=seg.data_ptr() + 2), dict(cen=cen.data_ptr() + 1), dict(cnt=cnt.data_ptr() + 2), dict(ws=ws.data_ptr() + 1),
           dict(rows=2 * 4096, cols=2 * 2048 * 4, S=2, G=0, g=None)]          # N = 2^24
    for change in bad:
        assert call(dict(ok, **change)) == -1, change
    torch.cuda.synchronize()
    assert (seg == -7).all() and (cen == 7.0).all() and (cnt == -7).all()      # nothing was launched
    assert lib.cmlpl_sp_workspace_bytes(0, 5, 3, 4) == 0 and lib.cmlpl_sp_workspace_bytes(5, 5, 9, 4) == 0
    assert lib.cmlpl_sp_workspace_bytes(5, 5, 3, 1) == 0 and lib.cmlpl_sp_workspace_bytes(5, 5, 3, 65) == 0
    for change in (dict(), dict(G=0, g=None), dict(cen=None, cnt=None), dict(gs=3), dict(nb=lib.cmlpl_sp_workspace_bytes(rows, cols, 3, 4))):
        assert call(dict(ok, **change)) == 0, change
    torch.cuda.synchronize()
    assert ((seg >= 0) & (seg < 9)).all()

    # the votes
    N = 9
    p = torch.rand(n, K, device=DEV)
    src = torch.randint(0, K, (n,), device=DEV)
    out = torch.full((n, K), 7.0, device=DEV)
    lab = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    sums = torch.full((N, K), -7, dtype=torch.int64, device=DEV)
    vws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    need = lib.cmlpl_sp_vote_workspace_bytes(N, K)
    assert need == 12 * N * (K + 2) and lib.cmlpl_sp_vote_workspace_bytes(0, K) == 0 and lib.cmlpl_sp_vote_workspace_bytes(N, 65) == 0
    okv = dict(seg=seg.data_ptr(), src=None, n=n, K=K, N=N, out=out.data_ptr(), lab=lab.data_ptr(), conf=None, ent=None,
               sums=sums.data_ptr(), cnt=None, sq=None, sl=None, ws=vws.data_ptr(), nb=4096)
    for fn, source in ((lib.cmlpl_sp_vote_probs, p), (lib.cmlpl_sp_vote_labels, src)):
        okv["src"] = source.data_ptr()
        callv = lambda a: fn(a["seg"], a["src"], a["n"], a["K"], a["N"], a["out"], a["lab"], a["conf"], a["ent"], a["sums"], a["cnt"],
                             a["sq"], a["sl"], a["ws"], a["nb"], st)
        badv = [dict(n=0), dict(N=0), dict(K=0), dict(K=65), dict(N=2 ** 30, K=64), dict(seg=None), dict(src=None), dict(ws=None),
                dict(nb=need - 1), dict(out=None, lab=None, sums=None), dict(seg=seg.data_ptr() + 2), dict(src=source.data_ptr() + 2),
                dict(out=out.data_ptr() + 2), dict(lab=lab.data_ptr() + 4), dict(conf=out.data_ptr() + 1), dict(ent=out.data_ptr() + 3),
                dict(sums=sums.data_ptr() + 4), dict(cnt=sums.data_ptr() + 4), dict(sq=out.data_ptr() + 2), dict(sl=lab.data_ptr() + 4),
                dict(ws=vws.data_ptr() + 4)]
        for change in badv:
            assert callv(dict(okv, **change)) == -1, change
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (lab == -7).all() and (sums == -7).all()
        for change in (dict(), dict(out=None), dict(lab=None, out=None), dict(nb=need), dict(conf=out.data_ptr(), ent=out.data_ptr() + 4 * n, out=None)):
            assert callv(dict(okv, **change)) == 0, change
        torch.cuda.synchronize()
        assert ((lab >= 0) & (lab < K)).all() and int(sums.sum()) > 0
        out.fill_(7.0), lab.fill_(-7), sums.fill_(-7)
