"""GPU: the connected-region kernels (csrc/regions.hip) against the definitions restated on the host
(cmlpl_amd.regions.cc_label_host / sieve_host).  Every output is an integer the definitions fix -- comp, size, id, M, the
sieved map, the four counters of every pass -- so everything is held EXACTLY; conf is a gather and is held bit for bit.

The shapes: single rows and columns, a strip thinner than a tile, sizes that are no multiple of the 32 x 32 tile, one exact
multiple of it in both directions (64 x 64) and one pixel past it in both (65 x 65), and 96 x 96 = nine tiles.  The patterns
(tests/regions_cases.py): one component across every tile border, as many components as pixels, one-pixel paths through
many tiles (the longest parent chains), tortuous clusters near the percolation threshold, voids, values up to 2^31 - 1."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from cmlpl_amd.regions import Sieve, cc_label_host, components, connect_segments, connect_segments_host, sieve, sieve_host
from tests.gpu_util import DEV
from tests.regions_cases import PATTERNS, pattern

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (3, 50), (33, 65), (64, 64), (65, 65), (61, 47), (96, 96)]
SIEVE_SHAPES = [(1, 1), (1, 70), (70, 1), (3, 50), (33, 65), (64, 64), (65, 65), (61, 47)]
SIEVE_PATTERNS = ("smoothed", "random2", "random9", "voids", "large_values", "checker", "all_void")


@functools.lru_cache(maxsize=None)
def _label_ref(name, rows, cols, conn):
    return cc_label_host(pattern(name, rows, cols, 7), rows, cols, conn)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_the_components_are_the_definitions(rows, cols, conn):
    for name in PATTERNS:
        v = pattern(name, rows, cols, 7)
        ref = _label_ref(name, rows, cols, conn)
        got = components(torch.from_numpy(v).to(DEV), rows, cols, conn, sizes=True, ids=True)
        torch.cuda.synchronize()
        tag = "%s %d x %d conn %d" % (name, rows, cols, conn)
        assert all(t.dtype == torch.int32 for t in (got.comp, got.size, got.id, got.M)), tag
        bad = int((got.comp.cpu().numpy() != ref["comp"]).sum())
        assert bad == 0, "%s: %d pixels with another root" % (tag, bad)
        assert np.array_equal(got.size.cpu().numpy(), ref["size"]), tag
        assert np.array_equal(got.id.cpu().numpy(), ref["id"]), tag
        assert got.count() == ref["M"], tag
    if rows * cols > 1:
        n = rows * cols
        assert _label_ref("constant", rows, cols, conn)["M"] == 1
        assert _label_ref("checker", rows, cols, conn)["M"] == (n if conn == 4 or min(rows, cols) == 1 else 2)
        assert _label_ref("all_void", rows, cols, conn)["M"] == 0


def test_the_optional_outputs_of_the_labelling():
    rows, cols = 61, 47
    v = torch.from_numpy(pattern("random2", rows, cols, 7)).to(DEV)
    ref = _label_ref("random2", rows, cols, 4)
    for sizes, ids in ((False, False), (True, False), (False, True)):
        got = components(v, rows, cols, 4, sizes=sizes, ids=ids)
        assert (got.size is not None) == sizes and (got.id is not None) == ids
        assert np.array_equal(got.comp.cpu().numpy(), ref["comp"]) and got.count() == ref["M"]
        assert not sizes or np.array_equal(got.size.cpu().numpy(), ref["size"])
        assert not ids or np.array_equal(got.id.cpu().numpy(), ref["id"])


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("rows,cols", SIEVE_SHAPES)
def test_the_sieve_is_the_definition(rows, cols, conn):
    n = rows * cols
    for name in SIEVE_PATTERNS:
        v = pattern(name, rows, cols, 7)
        vt = torch.from_numpy(v).to(DEV)
        for min_size in (1, 2, 4, 16, n + 1):
            for passes in (1, 4):
                ref = sieve_host(v, rows, cols, min_size, conn, passes)
                got = sieve(vt, rows, cols, Sieve(min_size, conn, passes))
                tag = "%s %d x %d conn %d min_size %d passes %d" % (name, rows, cols, conn, min_size, passes)
                assert got.labels.dtype == torch.int32 and got.stats.dtype == torch.int32 and got.conf is None, tag
                assert np.array_equal(got.stats.cpu().numpy(), ref["stats"]), tag         # word for word
                bad = int((got.labels.cpu().numpy() != ref["out"]).sum())
                assert bad == 0, "%s: %d pixels differ" % (tag, bad)
                if min_size == 1:
                    assert got.labels.cpu().numpy().tobytes() == v.tobytes(), tag
    assert np.array_equal(vt.cpu().numpy(), v)                    # the input is not written


def test_conf_is_the_gather_and_int64_labels_come_back_as_int64():
    rows, cols, K = 61, 47, 9
    n = rows * cols
    v = pattern("smoothed", rows, cols, 7).astype(np.int64)
    v[5] = -1                                                     # void, and two 2 x 2 blocks (large: they stay) of values
    v[[77, 78, 77 + cols, 78 + cols]] = K                         # that are no class: no probability of its own, NaN
    v[[n - 1, n - 2, n - 1 - cols, n - 2 - cols]] = K + 3
    rng = np.random.default_rng(3)
    p = rng.random((n, K)).astype(np.float32)
    p[11, 2] = np.nan
    ref = sieve_host(v, rows, cols, 4, 4, 4)
    got = sieve(torch.from_numpy(v).to(DEV), rows, cols, Sieve(4), probs=torch.from_numpy(p).to(DEV))
    out = got.labels.cpu().numpy()
    assert got.labels.dtype == torch.int64 and np.array_equal(out, ref["out"])
    ok = (out >= 0) & (out < K)
    want = np.where(ok, p[np.arange(n), np.where(ok, out, 0)], np.float32(np.nan)).astype(np.float32)
    assert np.array_equal(_bits(got.conf.cpu().numpy()), _bits(want)) and int((~ok).sum()) == 9
    assert got.summary()["relabelled"] == int(ref["stats"][:, 3].sum()) and got.summary()["components"] == int(ref["stats"][0, 0])


def _raw(lib, st, v, rows, cols, conn, min_size, passes, out, stats, ws, nbytes, probs=None, K=0, conf=None):
    return lib.cmlpl_cc_sieve(v.data_ptr(), rows, cols, conn, min_size, passes, out.data_ptr(), None if stats is None else
                              stats.data_ptr(), None if probs is None else probs.data_ptr(), K, None if conf is None else
                              conf.data_ptr(), ws.data_ptr(), nbytes, st)


def test_in_place_two_plus_two_and_whatever_the_workspace_held():
    from cmlpl_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, cols, conn = 65, 65, 8
    n = rows * cols
    nbytes = lib.cmlpl_cc_workspace_bytes(rows, cols)
    assert nbytes == 8 + 16 * n + 4 * ((n + 1023) // 1024 + 2) + 272
    for name in ("random2", "smoothed"):
        v = pattern(name, rows, cols, 7)
        ref4, ref2 = sieve_host(v, rows, cols, 4, conn, 4), sieve_host(v, rows, cols, 4, conn, 2)
        lref = cc_label_host(v, rows, cols, conn)
        outs = []
        for fill in (0x00, 0xFF, 0x7F):
            ws = torch.full((nbytes + 16,), fill, dtype=torch.uint8, device=DEV)
            vt = torch.from_numpy(np.concatenate([v, [-7]]).astype(np.int32)).to(DEV)
            stats = torch.full((4 * 4 + 1,), -7, dtype=torch.int32, device=DEV)
            assert _raw(lib, st, vt, rows, cols, conn, 4, 4, vt, stats, ws, nbytes) == 0           # d_out == d_map
            comp, size, ident = (torch.full((n + 1,), -7, dtype=torch.int32, device=DEV) for _ in range(3))
            M = torch.full((2,), -7, dtype=torch.int32, device=DEV)
            v0 = torch.from_numpy(v).to(DEV)
            assert lib.cmlpl_cc_label(v0.data_ptr(), rows, cols, conn, comp.data_ptr(), size.data_ptr(), ident.data_ptr(),
                                      M.data_ptr(), ws.data_ptr(), nbytes, st) == 0
            torch.cuda.synchronize()
            assert vt[-1] == -7 and stats[-1] == -7 and (ws[nbytes:] == fill).all()                 # nothing past the ends
            assert comp[-1] == -7 and size[-1] == -7 and ident[-1] == -7 and M.tolist() == [lref["M"], -7]
            outs.append([t.cpu().numpy() for t in (vt, stats, comp, size, ident)])
        for o in outs[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(o, outs[0]))
        assert np.array_equal(outs[0][0][:-1], ref4["out"]) and np.array_equal(outs[0][1][:-1].reshape(4, 4), ref4["stats"])
        assert np.array_equal(outs[0][2][:-1], lref["comp"]) and np.array_equal(outs[0][3][:-1], lref["size"])
        assert np.array_equal(outs[0][4][:-1], lref["id"])
        # 2 + 2 passes are the bytes of 4; the stats and the workspace's alignment slack are optional
        a = sieve(torch.from_numpy(v).to(DEV), rows, cols, Sieve(4, conn, 2))
        b = sieve(a.labels, rows, cols, Sieve(4, conn, 2))
        assert np.array_equal(a.labels.cpu().numpy(), ref2["out"])
        assert b.labels.cpu().numpy().tobytes() == ref4["out"].tobytes()
        assert np.array_equal(np.concatenate([a.stats.cpu().numpy(), b.stats.cpu().numpy()]), ref4["stats"])
        ws = torch.zeros(nbytes + 8, dtype=torch.uint8, device=DEV)
        out = torch.empty(n, dtype=torch.int32, device=DEV)
        assert _raw(lib, st, torch.from_numpy(v).to(DEV), rows, cols, conn, 4, 4, out, None, ws[4:], nbytes) == 0
        assert np.array_equal(out.cpu().numpy(), ref4["out"])


def test_a_call_captured_in_a_graph_replays_the_eager_bytes():
    rows, cols, K = 61, 47, 9
    n = rows * cols
    v = torch.from_numpy(pattern("smoothed", rows, cols, 7)).to(DEV)
    p = torch.rand(n, K, device=DEV)
    sv = Sieve(4, 8, 4)
    eager, ecc = sieve(v, rows, cols, sv, probs=p), components(v, rows, cols, 8, sizes=True, ids=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res, cc = sieve(v, rows, cols, sv, probs=p), components(v, rows, cols, 8, sizes=True, ids=True)
    g.replay()
    torch.cuda.synchronize()
    for a, b in ((res.labels, eager.labels), (res.stats, eager.stats), (res.conf, eager.conf), (cc.comp, ecc.comp),
                 (cc.size, ecc.size), (cc.id, ecc.id), (cc.M, ecc.M)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_the_library_refuses_what_it_cannot_take():
    from cmlpl_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, cols, K = 12, 9, 5
    n = rows * cols
    v = torch.randint(0, 3, (n,), dtype=torch.int32, device=DEV)
    out, comp, size, ident = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for _ in range(4))
    M = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    stats = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    p = torch.rand(n, K, device=DEV)
    conf = torch.full((n,), 7.0, device=DEV)
    need = lib.cmlpl_cc_workspace_bytes(rows, cols)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    assert lib.cmlpl_cc_workspace_bytes(0, 5) == 0 and lib.cmlpl_cc_workspace_bytes(5, -1) == 0
    assert lib.cmlpl_cc_workspace_bytes(65536, 32768) == 0 and lib.cmlpl_cc_workspace_bytes(2 ** 31 - 1, 1) > 0
    okl = dict(v=v.data_ptr(), rows=rows, cols=cols, conn=4, comp=comp.data_ptr(), size=size.data_ptr(), id=ident.data_ptr(),
               M=M.data_ptr(), ws=ws.data_ptr(), nb=need)
    label = lambda a: lib.cmlpl_cc_label(a["v"], a["rows"], a["cols"], a["conn"], a["comp"], a["size"], a["id"], a["M"], a["ws"],
                                         a["nb"], st)
    for change in (dict(rows=0), dict(cols=0), dict(rows=65536, cols=32768), dict(conn=6), dict(conn=0), dict(v=None),
                   dict(comp=None), dict(ws=None), dict(nb=need - 1), dict(v=v.data_ptr() + 2), dict(comp=comp.data_ptr() + 1),
                   dict(size=size.data_ptr() + 2), dict(id=ident.data_ptr() + 3), dict(M=M.data_ptr() + 2),
                   dict(ws=ws.data_ptr() + 1)):
        assert label(dict(okl, **change)) == -1, change
    oks = dict(v=v.data_ptr(), rows=rows, cols=cols, conn=8, ms=4, T=2, out=out.data_ptr(), stats=stats.data_ptr(), p=p.data_ptr(),
               K=K, conf=conf.data_ptr(), ws=ws.data_ptr(), nb=need)
    sv = lambda a: lib.cmlpl_cc_sieve(a["v"], a["rows"], a["cols"], a["conn"], a["ms"], a["T"], a["out"], a["stats"], a["p"], a["K"],
                                      a["conf"], a["ws"], a["nb"], st)
    for change in (dict(rows=0), dict(cols=-3), dict(rows=65536, cols=32768), dict(conn=5), dict(ms=0), dict(ms=-1), dict(T=0),
                   dict(T=17), dict(v=None), dict(out=None), dict(ws=None), dict(nb=need - 1), dict(p=None), dict(conf=None),
                   dict(K=0), dict(v=v.data_ptr() + 2), dict(out=out.data_ptr() + 2), dict(stats=stats.data_ptr() + 1),
                   dict(p=p.data_ptr() + 2), dict(conf=conf.data_ptr() + 3), dict(ws=ws.data_ptr() + 2)):
        assert sv(dict(oks, **change)) == -1, change
    torch.cuda.synchronize()
    for t in (out, comp, size, ident, M, stats):                  # nothing was launched
        assert (t == -7).all()
    assert (conf == 7.0).all()
    for change in (dict(), dict(size=None, id=None, M=None), dict(conn=8), dict(ws=ws.data_ptr() + 4)):
        assert label(dict(okl, **change)) == 0, change
    for change in (dict(), dict(stats=None), dict(p=None, conf=None, K=0), dict(ms=2 ** 31 - 1, T=16), dict(out=v.data_ptr())):
        assert sv(dict(oks, **change)) == 0, change
    torch.cuda.synchronize()
    assert (comp >= 0).all() and (conf != 7.0).all()


def test_connected_superpixels_vote_as_the_host_says():
    """Superpixel(connect=True) against connect_segments of segment_host + region_vote_host, exact as in
    tests/test_gpu_superpixel.py; the entropy by that file's allowance rule (8 x the error of the same fp32 chain on the host
    against fp64 on the same q)."""
    from cmlpl_amd.superpixel import Superpixel, region_vote_host, segment_host, superpixel_probs
    from tests.test_gpu_superpixel import _entropy64
    from tests.test_smooth_host import case
    rows, cols, K, S = 61, 47, 9, 6
    p, cube, _ = case(rows, cols, K, 3, 1, channels=7)
    seg = segment_host(cube, S, 1.0, 10, 3)["seg"]
    ids, M = connect_segments_host(seg, rows, cols, max(1, S * S // 4), 4, 4)
    ct, pt = torch.from_numpy(cube).to(DEV), torch.from_numpy(p).to(DEV)
    got_ids, got_M = connect_segments(torch.from_numpy(seg).to(DEV), rows, cols, S * S // 4)
    assert got_M == M and np.array_equal(got_ids.cpu().numpy(), ids)
    for vote in ("soft", "hard"):
        res = superpixel_probs(pt, ct, Superpixel(S, vote=vote, connect=True), conf=True, entropy=True)
        torch.cuda.synchronize()
        assert res.M == M and np.array_equal(res.connected.cpu().numpy(), ids) and np.array_equal(res.segments.seg.cpu().numpy(), seg)
        want = region_vote_host(ids, M, K, **(dict(probs=p) if vote == "soft" else dict(labels=p.argmax(1))))
        assert np.array_equal(res.sums.cpu().numpy(), want["P"]) and np.array_equal(res.seg_counts.cpu().numpy(), want["cnt"])
        assert np.array_equal(res.labels.cpu().numpy(), want["labels"])
        assert np.array_equal(_bits(res.probs.cpu().numpy()), _bits(want["probs"]))
        assert np.array_equal(_bits(res.conf.cpu().numpy()), _bits(want["conf"]))
        assert (want["cnt"] > 0).all()                            # every connected segment has pixels
        e64 = _entropy64(want["probs"])
        yard, err = float(np.abs(want["entropy"] - e64).max()), float(np.abs(res.entropy.cpu().numpy() - e64).max())
        print("connected %s: M %d, entropy err %.2e (allowed %.2e)" % (vote, M, err, 8 * yard))
        assert err <= 8 * yard
    plain = superpixel_probs(pt, ct, Superpixel(S), conf=True)
    assert plain.connected is None and plain.M is None
