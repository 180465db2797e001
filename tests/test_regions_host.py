"""CPU: the definitions of a component map and of a sieved map as cmlpl_amd.regions restates them (cc_label_host, sieve_host,
connect_segments_host) -- against scipy.ndimage.label where scipy imports, against the consequences the header lists, and on
the smoothed maps of tests/test_smooth_host.py's case builder, where the sieve has to raise the accuracy at min_size 4 and
is shown to lower it at min_size 16 (the regions of those cases are 7 pixels wide)."""
import os

import numpy as np
import pytest

from cmlpl_amd.regions import Sieve, cc_label_host, connect_segments_host, sieve_host
from tests.regions_cases import PATTERNS, pattern, smoothed_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OA_CASES = [(37, 29, 9, 3, 2), (61, 47, 9, 3, 2), (40, 23, 64, 3, 3)]      # (rows, cols, K, G, smoothing radius), seed 1


@pytest.mark.parametrize("conn", [4, 8])
def test_components_against_scipy_per_value(conn):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if conn == 8 else None
    for name in PATTERNS:
        rows, cols = (33, 65) if name != "all_void" else (9, 11)
        v = pattern(name, rows, cols, 3)
        cc = cc_label_host(v, rows, cols, conn)
        comp = np.full(rows * cols, -1, np.int64)
        for value in np.unique(v[v >= 0]):
            lab, m = ndi.label((v == value).reshape(rows, cols), structure)
            lab = lab.reshape(-1)
            first = np.full(m + 1, rows * cols, np.int64)
            np.minimum.at(first, lab, np.arange(rows * cols))
            comp[lab > 0] = first[lab[lab > 0]]
        assert np.array_equal(cc["comp"], comp), (name, conn)
        roots = np.flatnonzero(comp == np.arange(rows * cols))
        assert cc["M"] == len(roots)
        assert np.array_equal(cc["id"][roots], np.arange(len(roots)))            # numbered in first-pixel order
        inside = comp >= 0
        assert np.array_equal(cc["id"][inside], cc["id"][comp[inside]]) and (cc["id"][~inside] == -1).all()
        assert np.array_equal(cc["size"][inside], np.bincount(comp[inside], minlength=rows * cols)[comp[inside]])
        assert (cc["size"][~inside] == 0).all()


def test_known_small_maps():
    v = np.array([[1, 1, 0], [0, 1, 0], [1, 0, -1]], np.int32).reshape(-1)
    c4, c8 = cc_label_host(v, 3, 3, 4), cc_label_host(v, 3, 3, 8)
    assert c4["comp"].tolist() == [0, 0, 2, 3, 0, 2, 6, 7, -1] and c4["M"] == 5
    assert c4["size"].tolist() == [3, 3, 2, 1, 3, 2, 1, 1, 0] and c4["id"].tolist() == [0, 0, 1, 2, 0, 1, 3, 4, -1]
    assert c8["comp"].tolist() == [0, 0, 2, 2, 0, 2, 0, 2, -1] and c8["M"] == 2             # the diagonals join
    board = (np.add.outer(np.arange(6), np.arange(7)) % 2).astype(np.int32).reshape(-1)
    assert cc_label_host(board, 6, 7, 4)["M"] == 42 and cc_label_host(board, 6, 7, 8)["M"] == 2
    assert cc_label_host(np.full(12, -5), 3, 4, 4)["M"] == 0
    one = cc_label_host(np.full(12, 2 ** 31 - 1), 3, 4, 4)
    assert one["M"] == 1 and (one["comp"] == 0).all() and (one["size"] == 12).all()


def test_a_target_is_the_largest_large_neighbour_and_ties_go_to_the_smaller_root():
    # a lone pixel (value 9) between a region of 4 (value 1), one of 6 (value 2) and one of 6 (value 3, a later root)
    v = np.array([[1, 1, 2, 2, 2],
                  [1, 1, 9, 2, 2],
                  [7, 3, 3, 3, 2],
                  [7, 3, 3, 3, 0]], np.int32).reshape(-1)
    r = sieve_host(v, 4, 5, 3, 4, 1)
    assert r["out"][7] == 2                                      # 2 and 3 both have six pixels: root 2 < root 11
    assert r["out"][10] == r["out"][15] == 3                     # the pair of 7s touches 1 (four pixels) and 3 (six)
    assert r["out"][19] == 2                                     # the lone 0: 2 and 3 tie again
    assert r["stats"].tolist() == [[6, 3, 3, 4]]                 # components, small, small with a target, pixels relabelled
    assert sieve_host(v, 4, 5, 3, 4, 2)["stats"][1].tolist() == [3, 0, 0, 0]
    # a small component with only small neighbours waits: two 1-pixel islands side by side in a void frame stay for ever
    w = np.array([-1, 4, 5, -1], np.int32)
    rr = sieve_host(w, 1, 4, 2, 4, 3)
    assert rr["out"].tolist() == w.tolist() and rr["stats"][:, 2:].sum() == 0
    # void is never a target and never changes
    z = np.array([-3, 1, -3, 2, 2, 2], np.int32)
    assert sieve_host(z, 1, 6, 2, 4, 2)["out"].tolist() == [-3, 1, -3, 2, 2, 2]
    assert sieve_host(z, 1, 6, 2, 8, 2)["out"].tolist() == [-3, 1, -3, 2, 2, 2]


@pytest.mark.parametrize("conn", [4, 8])
def test_the_consequences_of_the_definition(conn):
    rows, cols = 37, 29
    for name in ("smoothed", "random2", "random9", "voids"):
        v = pattern(name, rows, cols, 5)
        n = rows * cols
        assert sieve_host(v, rows, cols, 1, conn, 3)["out"].tobytes() == v.astype(np.int32).tobytes()      # min_size 1
        prev, u = None, v
        four = sieve_host(v, rows, cols, 4, conn, 4)
        for t in range(4):                                       # T passes in one call = the same passes in several calls
            before = cc_label_host(u, rows, cols, conn)
            step = sieve_host(u, rows, cols, 4, conn, 1)
            assert step["stats"][0].tolist() == four["stats"][t].tolist(), (name, t)
            after = cc_label_host(step["out"], rows, cols, conn)
            large = before["size"] >= 4
            assert np.array_equal(step["out"][large], u[large])                  # only small components move
            assert (after["size"][large] >= before["size"][large]).all()         # large components only grow
            changed = step["out"] != u
            assert int(changed.sum()) == step["stats"][0][3]
            if prev is not None:
                assert not (changed & prev).any()                                # a relabelled pixel never changes again
            prev = changed if prev is None else (prev | changed)
            if step["stats"][0][3] == 0:
                assert step["out"].tobytes() == u.tobytes()
            assert (step["out"][v < 0] == v[v < 0]).all()
            u = step["out"]
        assert u.tobytes() == four["out"].tobytes()
        zero = np.flatnonzero(four["stats"][:, 3] == 0)
        if len(zero):                                            # a pass that moves nothing makes the later ones the identity
            assert (four["stats"][zero[0]:, 3] == 0).all() and (four["stats"][zero[0]:, 0] == four["stats"][zero[0], 0]).all()
        everything = sieve_host(v, rows, cols, n + 1, conn, 2)   # nothing is large: nothing has a target
        assert everything["out"].tobytes() == v.astype(np.int32).tobytes() and everything["stats"][:, 2:].sum() == 0


@pytest.mark.parametrize("rows,cols,K,G,R", OA_CASES)
def test_the_sieve_raises_the_accuracy_of_a_smoothed_map(rows, cols, K, G, R):
    lab, Y = smoothed_case(rows, cols, K, G, R)
    out = sieve_host(lab, rows, cols, 4, 4, 4)
    before, after = (lab == Y).mean(), (out["out"] == Y).mean()
    print("%d x %d x %d R %d: OA %.3f -> %.3f, relabelled %s, components %d -> %d" % (
        rows, cols, K, R, before, after, out["stats"][:, 3].tolist(), out["stats"][0, 0],
        cc_label_host(out["out"], rows, cols, 4)["M"]))
    assert after > before


def test_a_min_size_near_the_regions_width_lowers_the_accuracy():
    """the risk: the regions of these cases are 7 pixels wide, and a clipped one at the scene's edge has fewer than 16 pixels"""
    lowered = []
    for rows, cols, K, G, R in OA_CASES:
        lab, Y = smoothed_case(rows, cols, K, G, R)
        four = (sieve_host(lab, rows, cols, 4, 4, 4)["out"] == Y).mean()
        sixteen = (sieve_host(lab, rows, cols, 16, 4, 4)["out"] == Y).mean()
        print("%d x %d x %d: OA min_size 4 %.3f, min_size 16 %.3f" % (rows, cols, K, four, sixteen))
        lowered.append(sixteen < four)
    assert any(lowered)


@pytest.mark.parametrize("rows,cols,S", [(37, 29, 4), (37, 29, 6), (61, 47, 8)])
def test_connected_segments(rows, cols, S):
    """Every output id is one component, the ids are 0 .. M - 1 in first-pixel order, and M >= the number of input segments
    that own a component of at least min_size pixels: such a component never moves, and no other segment's pixels can take
    its id's place.  The plain count of non-empty input segments is NOT a lower bound in general -- a segment all of whose
    fragments are small is handed over whole (37 x 29, S 4: 80 non-empty segments, some of a single pixel, 75 after) --, so
    it is asserted where every non-empty segment owns a large component."""
    from cmlpl_amd.superpixel import segment_host
    from tests.test_smooth_host import case
    _, cube, _ = case(rows, cols, 4, 3, 1, channels=5)
    seg = segment_host(cube, S, 1.0, 10, 3)["seg"]
    min_size, n = max(1, S * S // 4), rows * cols
    nonempty = len(np.unique(seg))
    for conn in (4, 8):
        ids, M = connect_segments_host(seg, rows, cols, min_size, conn, 4)
        cc = cc_label_host(ids, rows, cols, conn)
        assert cc["M"] == M and np.array_equal(cc["id"], ids)                    # every id's pixels form ONE component
        firsts = np.full(M, n, np.int64)
        np.minimum.at(firsts, ids, np.arange(n))
        assert ids.min() == 0 and ids.max() == M - 1 and (np.diff(firsts) > 0).all()     # 0 .. M - 1 in first-pixel order
        before = cc_label_host(seg, rows, cols, conn)
        keep = len(np.unique(seg[before["size"] >= min_size]))
        print("%d x %d S %d conn %d: %d segments (%d with a large component), %d components -> %d connected segments" % (
            rows, cols, S, conn, nonempty, keep, before["M"], M))
        assert keep <= M <= before["M"]
        if keep == nonempty:
            assert M >= nonempty


def test_sieve_validation():
    assert Sieve(4).params() == (4, 4, 4) and Sieve(1, 8, 16).params() == (1, 8, 16)
    for bad in (Sieve(0), Sieve(2 ** 31), Sieve(4, 6), Sieve(4, 4, 0), Sieve(4, 4, 17)):
        with pytest.raises(ValueError):
            bad.params()
    with pytest.raises(ValueError):
        cc_label_host(np.zeros(5), 2, 3, 4)
    with pytest.raises(ValueError):
        cc_label_host(np.zeros(6), 2, 3, 6)


def test_the_source_is_built_and_the_header_declares_the_exports():
    from cmlpl_amd import _lib, build_ext
    names = ("cmlpl_cc_workspace_bytes", "cmlpl_cc_label", "cmlpl_cc_sieve")
    assert "regions.hip" in build_ext.SOURCES and all(n in _lib.EXPORTS for n in names)
    header = open(os.path.join(ROOT, "include", "cmlpl.h")).read()
    assert all(n + "(" in header for n in names)
    assert "THE DEFINITION OF A COMPONENT MAP" in header and "THE DEFINITION OF A SIEVED MAP" in header
    import cmlpl_amd
    assert cmlpl_amd.Sieve is Sieve and cmlpl_amd.cc_label_host is cc_label_host


def test_superpixel_keeps_its_five_params_and_gains_connect():
    from cmlpl_amd.superpixel import Superpixel
    assert Superpixel(4).connect is False and Superpixel(4, connect=True).connect is True
    assert Superpixel(4, connect=True).params() == Superpixel(4).params() and len(Superpixel(4).params()) == 5
    assert Superpixel._fields[-1] == "connect"


def test_parsers_take_the_flags_and_refuse_what_they_cannot_mean():
    import predict
    import train
    from scene_report import Stage, sieve_stage
    tp, pp = train.build_parser(), predict.build_parser()
    a = tp.parse_args(["--sieve", "4", "--sieve_conn", "8", "--superpixel", "4", "--sp_connect"])
    assert train.sieve_of(a) == Sieve(4, 8) and train.superpixel_of(a).connect is True
    assert train.sieve_of(tp.parse_args([])) is None and train.superpixel_of(tp.parse_args(["--superpixel", "4"])).connect is False
    saved = train.saved_args(a)
    assert not any(k.startswith(("sieve", "sp_")) for k in saved) and saved == train.saved_args(tp.parse_args([]))
    for argv, word in ((["--sieve_passes", "2"], "belongs to --sieve"), (["--sieve", "0"], "min_size"), (["--sieve", "4", "--sieve_passes", "17"], "passes"),
                       (["--sp_connect"], "belongs to --superpixel")):
        with pytest.raises(SystemExit) as e:
            train.sieve_of(tp.parse_args(argv)), train.superpixel_of(tp.parse_args(argv))
        assert word in str(e.value), argv
    base = ["--ckpt", "x.pt", "--net", "ensemble"]
    for argv, word in ((["--sieve", "4", "--entropy", "e.npy"], "--entropy together with --sieve"),
                       (["--sieve", "4", "--net", "both"], "--net both"), (["--sieve", "4", "--knn", "3"], "--knn")):
        with pytest.raises(SystemExit) as e:
            predict.check_args(pp.parse_args(base + argv))
        assert word in str(e.value), argv
    ok = pp.parse_args(base + ["--sieve", "4", "--smooth", "2", "--superpixel", "4", "--temperature", "2", "--confidence", "c.npy"])
    predict.check_args(ok)
    assert [name for name, _ in predict.plan(ok, True).stages] == ["smooth", "superpixel", "temper", "sieve"]       # LAST
    assert predict.plan(pp.parse_args(base), True).stages == ()
    stage = sieve_stage(Sieve(4))
    assert stage.suffix == "_sv" and stage.scored is False and Stage("t", "_x", None).scored is True
