"""CPU: the definitions of a superpixel map and of a region vote (include/cmlpl.h) as ``cmlpl_amd.superpixel`` restates them
in numpy -- what they promise on the case builder of tests/test_smooth_host.py (regions 7 pixels wide, guide = the class's
prototype + 0.5 N(0,1)), their edge cases, and the wiring of the feature that needs no device: ``Superpixel``, the source
list, the header, the export list, the two command lines' refusals.

The figures of the first test were observed before the kernels existed (raw OA / region-vote OA / ASA): 0.425 / 0.955 /
0.989 on 37 x 29 at S 4 and 0.443 / 0.985 / 0.985 on 61 x 47 at S 6; the bounds asserted are 0.5 / 0.9 / 0.95."""
import os
import re

import numpy as np
import pytest
import torch

from cmlpl_amd.superpixel import Superpixel, asa, asa_of_sums, compact_weight, region_vote_host, segment_host
from tests.test_smooth_host import case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def regular(cube, G):
    g = cube[:, :, :G].reshape(cube.shape[0] * cube.shape[1], G)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(g) & (np.abs(g) <= 2.0 ** 20)).all(1)


def check_map(h, cube, S, G):
    """what every map promises: labels in range, counts of the regular pixels, a segment inside its 3 x 3 block of cells"""
    rows, cols = cube.shape[:2]
    N = h["ny"] * h["nx"]
    seg, counts = h["seg"], h["counts"]
    assert seg.dtype == np.int32 and seg.shape == (rows * cols,) and counts.dtype == np.int32 and counts.shape == (N,)
    assert h["centres"].dtype == np.float32 and h["centres"].shape == (N, 2 + G)
    assert (h["ny"], h["nx"]) == (-(-rows // S), -(-cols // S))
    assert ((seg >= 0) & (seg < N)).all()
    reg = regular(cube, G)
    assert counts.sum() == reg.sum() and np.array_equal(counts, np.bincount(seg[reg], minlength=N))
    assert counts.max() <= 9 * S * S
    yy, xx = np.divmod(np.arange(rows * cols), cols)
    assert (np.abs(yy // S - seg // h["nx"]) <= 1).all() and (np.abs(xx // S - seg % h["nx"]) <= 1).all()
    assert np.isfinite(h["centres"]).all()
    return N


@pytest.mark.parametrize("rows,cols,K,S", [(37, 29, 9, 4), (61, 47, 9, 6)])
def test_the_region_vote_on_the_builders_cases(rows, cols, K, S):
    p, cube, Y = case(rows, cols, K, 3, 1)
    h = segment_host(cube, S, 1.0, 10, 3)
    N = check_map(h, cube, S, 3)
    v = region_vote_host(h["seg"], N, K, probs=p)
    raw, oa = (p.argmax(1) == Y).mean(), (v["labels"] == Y).mean()
    bound = asa(h["seg"], N, np.arange(rows * cols), Y, K)
    print("%d x %d K %d S %d: OA raw %.3f region vote %.3f ASA %.3f, changed per iteration %s, empty %d"
          % (rows, cols, K, S, raw, oa, bound, h["changed"], (h["counts"] == 0).sum()))
    assert raw <= 0.5 and oa >= 0.9 and bound >= 0.95
    assert oa <= bound
    assert (h["counts"] > 0).all()
    hard = region_vote_host(h["seg"], N, K, labels=p.argmax(1))
    assert (hard["labels"] == Y).mean() <= bound


@pytest.mark.parametrize("rows,cols,K,S", [(40, 23, 64, 4), (61, 47, 16, 8)])
def test_the_vote_never_exceeds_asa(rows, cols, K, S):
    p, cube, Y = case(rows, cols, K, 3, 1)
    h = segment_host(cube, S, 1.0, 10, 3)
    N = check_map(h, cube, S, 3)
    bound = asa(h["seg"], N, np.arange(rows * cols), Y, K)
    for v in (region_vote_host(h["seg"], N, K, probs=p), region_vote_host(h["seg"], N, K, labels=p.argmax(1))):
        assert (v["labels"] == Y).mean() <= bound
        assert (v["labels"] == Y).mean() > (p.argmax(1) == Y).mean()
    # ASA on a share of the pixels: the others hold -1 and are left out
    rows_ = np.arange(0, rows * cols, 3)
    tm = np.full(rows * cols, -1, np.int64)
    tm[rows_] = Y[rows_]
    t = region_vote_host(h["seg"], N, K, labels=tm)
    assert t["cnt"].sum() == len(rows_) and asa(h["seg"], N, rows_, Y[rows_], K) == asa_of_sums(t["P"])
    assert np.isnan(asa_of_sums(np.zeros((3, 2), np.int64)))


def test_an_irregular_pixel_keeps_its_own_cell_and_leaves_every_centre_finite():
    _, cube, _ = case(24, 20, 5, 3, 2, channels=6)
    cube[5, 6, 1] = np.nan
    cube[7, 7, 0] = 3e7
    cube[0, 0, 2] = -np.inf
    cube[9, 9, 4] = np.nan                  # (past the guide: never read)
    h = segment_host(cube, 4, 1.0, 10, 3)
    check_map(h, cube, 4, 3)
    nx = h["nx"]
    for y, x in ((5, 6), (7, 7), (0, 0)):
        assert h["seg"][y * 20 + x] == (y // 4) * nx + x // 4
    assert h["counts"].sum() == 24 * 20 - 3
    # the centre pixel of a cell irregular: its initial guide is zeros, and the first update replaces it
    cube[2, 2, 0] = np.nan
    one = segment_host(cube, 4, 1.0, 1, 3)
    check_map(one, cube, 4, 3)


@pytest.mark.parametrize("rows,cols,C,G,S", [(1, 1, 5, 3, 4), (3, 50, 5, 3, 8), (50, 3, 5, 0, 4), (9, 9, 12, 8, 2), (17, 13, 5, 3, 64)])
def test_shapes_at_the_edges(rows, cols, C, G, S):
    _, cube, _ = case(rows, cols, 4, G, 3, channels=C)
    h = segment_host(cube, S, 1.0, 10, G)
    N = check_map(h, cube, S, G)
    assert (h["counts"] > 0).all()
    if S == 64:
        assert N == 1 and (h["seg"] == 0).all() and h["counts"][0] == rows * cols
    if G == 0:              # no guide: the distance in the image alone -- every pixel stays with the nearest centre
        assert h["changed"][-1] == 0
    again = segment_host(cube, S, 1.0, 10, G)
    assert all(np.array_equal(h[k], again[k]) for k in ("seg", "centres", "counts"))
    legs = segment_host(cube, S, 1.0, 4, G)
    assert legs["changed"] == h["changed"][:4]


def test_exact_properties_of_the_vote():
    rng = np.random.default_rng(5)
    n, N, K = 200, 7, 5
    seg = rng.integers(0, N - 1, n).astype(np.int32)           # (segment N - 1 stays empty)
    p = rng.random((n, K)).astype(np.float32)
    p[3, 2], p[4, 0], p[5, 1], p[6, 4] = np.nan, -0.25, 2.5, np.inf
    seg[10], seg[11] = -1, N
    v = region_vote_host(seg, N, K, probs=p)
    valid = np.ones(n, bool)
    valid[[3, 4, 5, 6, 10, 11]] = False
    assert v["cnt"].sum() == valid.sum() and v["cnt"][N - 1] == 0
    assert v["seg_labels"][N - 1] == -1 and np.isnan(v["q"][N - 1]).all() and np.isnan(v["seg_entropy"][N - 1])
    assert v["labels"][10] == -1 and v["labels"][11] == -1 and np.isnan(v["probs"][[10, 11]]).all() and np.isnan(v["conf"][10])
    for i in (3, 4, 5, 6):                                      # an invalid row inside a voted segment is repaired by its region
        assert v["labels"][i] == v["seg_labels"][seg[i]] >= 0 and np.isfinite(v["probs"][i]).all()
    s = 2
    want = np.rint(p[valid & (seg == s)].astype(np.float64) * 2.0 ** 24).astype(np.int64).sum(0)
    assert np.array_equal(v["P"][s], want)
    assert np.array_equal(v["q"][s], (want / (v["cnt"][s] * 2.0 ** 24)).astype(np.float32))
    assert (v["seg_entropy"][:N - 1] >= 0).all() and np.array_equal(v["seg_conf"][:N - 1], v["q"][:N - 1].max(1))
    # equal tops: the lower index wins; a hard vote's q are exact quotients
    lab = np.array([3, 1, 3, 1, 0, 7, -1], np.int64)
    hv = region_vote_host(np.zeros(7, np.int32), 1, 4, labels=lab)
    assert hv["cnt"][0] == 5 and hv["P"][0].tolist() == [1, 2, 0, 2] and hv["seg_labels"][0] == 1
    assert hv["q"][0].tolist() == [np.float32(0.2), np.float32(0.4), 0.0, np.float32(0.4)] and (hv["labels"] == 1).all()
    assert compact_weight(1.0, 4) == np.float32(1 / 16) and compact_weight(3.0, 2) == np.float32(2.25)


# ------------------------------------------------------------------ wiring
def test_superpixel_validation():
    from cmlpl_amd.superpixel import region_vote, segment
    assert Superpixel(4).params() == (4, 1.0, 10, 3, "soft") and Superpixel(8, 2.5, 3, 8, "hard").params(5) == (8, 2.5, 3, 5, "hard")
    assert Superpixel(2, guide=0).params(60)[3] == 0 and Superpixel(64, iters=100).params()[2] == 100
    for bad in (Superpixel(1), Superpixel(65), Superpixel(4, compact=0.0), Superpixel(4, compact=-1.0), Superpixel(4, compact=float("inf")),
                Superpixel(4, compact=float("nan")), Superpixel(4, compact=1e-30), Superpixel(4, compact=1e30), Superpixel(4, iters=0),
                Superpixel(4, iters=101), Superpixel(4, guide=-1), Superpixel(4, guide=9), Superpixel(4, vote="majority")):
        with pytest.raises(ValueError, match="Superpixel"):
            bad.params()
    assert "not tuned" in Superpixel.__doc__.lower()
    with pytest.raises(ValueError, match="cuda"):
        segment(torch.zeros(3, 4, 5), Superpixel(2))
    with pytest.raises(ValueError, match="cuda"):
        region_vote(torch.zeros(12, dtype=torch.int32), probs=torch.zeros(12, 3), N=2)
    import cmlpl_amd
    for name in ("Superpixel", "segment", "region_vote", "superpixel_probs", "asa", "segment_host", "region_vote_host"):
        assert getattr(cmlpl_amd, name) is getattr(cmlpl_amd.superpixel, name)


def test_the_source_is_built_and_the_header_declares_the_exports():
    from cmlpl_amd import _lib, build_ext
    names = ("cmlpl_sp_workspace_bytes", "cmlpl_sp_segment", "cmlpl_sp_vote_workspace_bytes", "cmlpl_sp_vote_probs", "cmlpl_sp_vote_labels")
    assert "superpixel.hip" in build_ext.SOURCES and all(n in _lib.EXPORTS for n in names)
    assert os.path.exists(os.path.join(ROOT, "cmlpl_amd", "csrc", "superpixel.hip"))
    header = open(os.path.join(ROOT, "include", "cmlpl.h")).read()
    assert "#define CMLPL_ABI_VERSION 6" in header
    assert "THE DEFINITION OF A SUPERPIXEL MAP" in header and "THE DEFINITION OF A REGION VOTE" in header
    flat = " ".join(header.replace("*", " ").split())
    for phrase in ("d = g[ch] - c[ch]; dc2 = fmaf(d, d, dc2)", "ds2 = fmaf(dx, dx, fl(dy dy))", "D = fmaf(ds2, w, dc2)",
                   "a tie keeps the earlier candidate", "An irregular pixel computes nothing and keeps its own cell",
                   "n <= 9 S^2", "llrintf(g[ch] 2^24)", "llrintf(p[i][c] 2^24)", "ASA = sum_s max_c P[s][c] / sum_s cnt[s]"):
        assert phrase in flat, phrase
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    args = lambda fn: [a.split()[-1].lstrip("*") for a in re.search(r"\b%s\(([^;]*)\);" % fn, bare).group(1).split(",")]
    assert args("int cmlpl_sp_segment") == ["d_guide", "guide_stride", "G", "rows", "cols", "S", "m", "iters", "d_seg", "d_centres",
                                            "d_counts", "d_ws", "ws_bytes", "stream"]
    tail = ["n", "K", "N", "d_out_probs", "d_labels", "d_conf", "d_entropy", "d_sums", "d_cnt", "d_seg_probs", "d_seg_labels", "d_ws",
            "ws_bytes", "stream"]
    assert args("int cmlpl_sp_vote_probs") == ["d_seg", "d_probs", *tail]
    assert args("int cmlpl_sp_vote_labels") == ["d_seg", "d_src_labels", *tail]
    assert args("size_t cmlpl_sp_workspace_bytes") == ["rows", "cols", "G", "S"]
    # the new names come after everything that existed: nothing moves
    assert bare.index("cmlpl_sp_workspace_bytes") > bare.index("cmlpl_lp_propagate")


BADS = (["--superpixel", "1"], ["--superpixel", "65"], ["--superpixel", "4", "--sp_compact", "0"], ["--superpixel", "4", "--sp_compact", "nan"],
        ["--superpixel", "4", "--sp_iters", "0"], ["--superpixel", "4", "--sp_iters", "101"], ["--superpixel", "4", "--sp_guide", "9"],
        ["--sp_compact", "1"], ["--sp_iters", "3"], ["--sp_guide", "2"], ["--sp_vote", "hard"], ["--save_segments", "s.npy"])


def test_parsers_take_the_flags_and_refuse_what_they_cannot_mean():
    import predict
    import train
    q = predict.build_parser()
    a = q.parse_args(["--ckpt", "x"])
    assert (a.superpixel, a.sp_compact, a.sp_iters, a.sp_guide, a.sp_vote, a.save_segments) == (None,) * 6
    predict.check_args(a)
    for net in ("0", "1", "ema0", "ema1", "ensemble", "ensemble_all"):
        for more in ([], ["--tta", "2"], ["--smooth", "2", "--temperature", "2", "--reliability"]):
            predict.check_args(q.parse_args(["--ckpt", "x", "--net", net, "--superpixel", "4", "--sp_compact", "0.5", "--sp_iters", "3",
                                             "--sp_guide", "0", "--sp_vote", "hard", "--save_segments", "s.npy", "--proba", "p.npy", *more]))
    for net in ("both", "ema_both"):
        with pytest.raises(SystemExit) as e:
            predict.check_args(q.parse_args(["--ckpt", "x", "--net", net, "--superpixel", "4"]))
        assert "--net " + net in str(e.value) and "--superpixel" in str(e.value)
    for more in (["--knn", "3"], ["--embed", "e.npy"], ["--propagate"]):
        with pytest.raises(SystemExit) as e:
            predict.check_args(q.parse_args(["--ckpt", "x", "--superpixel", "4", *more]))
        assert "--superpixel" in str(e.value)
    with pytest.raises(SystemExit):
        q.parse_args(["--ckpt", "x", "--superpixel", "4", "--sp_vote", "majority"])
    for bad in BADS:
        with pytest.raises(SystemExit):
            predict.check_args(q.parse_args(["--ckpt", "x", *bad]))
    p = train.build_parser()
    assert train.superpixel_of(p.parse_args(["--synthetic", "B2"])) is None
    assert train.superpixel_of(p.parse_args(["--synthetic", "B2", "--superpixel", "4"])) == Superpixel(4)
    assert train.superpixel_of(p.parse_args(["--synthetic", "B2", "--superpixel", "8", "--sp_compact", "2", "--sp_iters", "5", "--sp_guide",
                                             "1", "--sp_vote", "hard"])) == Superpixel(8, 2.0, 5, 1, "hard")
    for bad in BADS:
        with pytest.raises(SystemExit):
            train.superpixel_of(p.parse_args(["--synthetic", "B2", *bad]))
    assert train.SP_TAG == "_sp"
    rel = p.parse_args(["--synthetic", "B2", "--reliability", "--superpixel", "4"])
    train.check_reliability_args(rel, None, train.superpixel_of(rel))      # the _sp block is one --reliability can score


def test_refusals_come_before_any_device_call(monkeypatch):
    import predict
    import train

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch.cuda, "set_device", boom)
    for bad in (["--net", "both", "--superpixel", "4"], ["--sp_guide", "2"], ["--superpixel", "4", "--knn", "3"]):
        with pytest.raises(SystemExit):
            predict.main(predict.build_parser().parse_args(["--ckpt", "nowhere.pt", *bad]))
    for bad in (["--sp_iters", "2"], ["--superpixel", "100"], ["--superpixel", "4", "--no_eval"]):
        with pytest.raises(SystemExit):
            train.main(train.build_parser().parse_args(["--synthetic", "B2", *bad]))
    monkeypatch.setenv("WORLD_SIZE", "2")                       # under the launcher: one GPU only
    with pytest.raises(SystemExit) as e:
        train.main(train.build_parser().parse_args(["--synthetic", "B2", "--superpixel", "4"]))
    assert "--superpixel" in str(e.value) and "one GPU" in str(e.value)


def test_saved_args_and_run_record_never_hold_the_flags():
    import train
    from cmlpl_amd import HyperParams
    from tests.test_gpu_ema import PARENT_ARGS, PARENT_RUN
    p = train.build_parser()
    a0 = p.parse_args(["--synthetic", "B2"])
    a1 = p.parse_args(["--synthetic", "B2", "--superpixel", "4", "--sp_guide", "1", "--sp_vote", "hard", "--save_segments", "s.npy"])
    s0, s1 = train.saved_args(a0), train.saved_args(a1)
    assert set(s0) == PARENT_ARGS and s1 == s0                  # never recorded in a checkpoint
    r0, r1 = (train.run_record(a, HyperParams(), train.SYNTH["B2"], False) for a in (a0, a1))
    assert r0 == r1 and set(r0) == PARENT_RUN
