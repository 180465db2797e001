"""CPU: the window-gather table (tests/window_cases.py) held without a device.

  1. Every regime of extract_patches_kernel / cube_feed_kernel / tta_patches_kernel that the table exists for is hit by at
     least two of its cases (one where the regime admits a single (C, w) -- said at the entry): someone who edits the table
     cannot silently drop a regime.  tests/test_gpu_window_envelope.py runs the same cases on the GPU.
  2. The kernels' division by a float reciprocal -- i = (int)(((float)t + 0.5f) * (1.0f / n4)), j = (int)(((float)e0 + 0.5f)
     * (1.0f / C)) -- restated in numpy float32, equals the integer quotient over the whole envelope the cut accepts.
  3. The table's reference for a spatial element (``spatial_index`` gathered from the oracle cut) is the window of the
     flipped / transposed scene at the mapped pixel: the reference itself is not a transposed g.
  4. Every case is a shape the kernel it names accepts (cmlpl_patches_fit; the feed's own LDS and make_dims' window)."""
import numpy as np
import pytest

from oracle import cmlpl_oracle as O
from tests import window_cases as W
from tests.window_cases import CASES, EXTRACT, FEED, TTA, LDS_MAX

MARGIN = [c for c in CASES if c.scene == "margin"]


def _v(c, key):
    return c.values()[key]


# name -> (predicate over a case, how many cases at least).  A regime that only one (C, w) can reach asks for one case.
REGIMES = {
    # ---- LDS layout of extract_patches_kernel, with C < 4 (a 16-byte item spans several pixels)
    "extract: odd layout, C < 4, 16-byte items": (lambda c: EXTRACT in c.kernels and c.C in (1, 3) and _v(c, "n4") > 0, 2),
    "extract: even layout, C < 4 (C = 2 is the only such C), 16-byte items":
        (lambda c: EXTRACT in c.kernels and c.C == 2 and _v(c, "n4") > 0, 2),
    "feed: C < 4": (lambda c: FEED in c.kernels and c.C < 4, 2),
    # ---- span tail
    "extract: rem 1": (lambda c: EXTRACT in c.kernels and _v(c, "rem") == 1 and _v(c, "n4") > 0, 2),
    "extract: rem 2, odd layout": (lambda c: EXTRACT in c.kernels and _v(c, "rem") == 2 and c.C & 1 and _v(c, "n4") > 0, 2),
    "extract: rem 2, even layout": (lambda c: EXTRACT in c.kernels and _v(c, "rem") == 2 and not c.C & 1 and _v(c, "n4") > 0, 2),
    "extract: rem 3": (lambda c: EXTRACT in c.kernels and _v(c, "rem") == 3 and _v(c, "n4") > 0, 2),
    "feed: rem 2": (lambda c: FEED in c.kernels and _v(c, "rem") == 2, 2),
    "feed: rem 3": (lambda c: FEED in c.kernels and _v(c, "rem") == 3, 2),
    # ---- n4 == 0
    "extract: n4 == 0": (lambda c: EXTRACT in c.kernels and _v(c, "n4") == 0, 2),
    "extract: n4 == 0, even layout (C = 2, w = 1 is the only one)": (lambda c: _v(c, "n4") == 0 and not c.C & 1, 1),
    # ---- more than one batch of items
    "extract: odd layout, more than one batch": (lambda c: EXTRACT in c.kernels and c.C & 1 and _v(c, "batches") > 1, 2),
    "extract: even layout, more than one batch": (lambda c: EXTRACT in c.kernels and not c.C & 1 and _v(c, "batches") > 1, 2),
    "feed: the t0 loop iterates": (lambda c: FEED in c.kernels and _v(c, "batches") > 1, 2),
    # ---- column-margin path: halves and passes
    "margin: C <= 64": (lambda c: FEED in c.kernels and c.C <= 64, 2),
    "margin: second half of the first pass (65 .. 128)": (lambda c: FEED in c.kernels and 64 < c.C <= 128, 2),
    "margin: first half of the second pass (129 .. 192)": (lambda c: FEED in c.kernels and 128 < c.C <= 192, 2),
    "margin: second half of the second pass (193 .. 256)": (lambda c: FEED in c.kernels and 192 < c.C <= 256, 2),
    "margin: extract with C in 193 .. 256": (lambda c: EXTRACT in c.kernels and 192 < c.C <= 256, 2),
    # ---- scatter and store
    "extract: w * w > 256 with odd C": (lambda c: EXTRACT in c.kernels and _v(c, "big") and c.C & 1, 2),
    "extract: w * w > 256 with even C": (lambda c: EXTRACT in c.kernels and _v(c, "big") and not c.C & 1, 1),
    "extract: C < 8, waves without a band": (lambda c: EXTRACT in c.kernels and c.C < 8 and _v(c, "n4") > 0, 2),
    "feed: per % 8 == 0": (lambda c: FEED in c.kernels and _v(c, "per8") == 0, 2),
    "feed: per % 8 != 0": (lambda c: FEED in c.kernels and _v(c, "per8") != 0, 2),
    "feed: per odd (rows on odd bases: unaligned 16-byte stores)": (lambda c: FEED in c.kernels and W.per(c.C, c.w) & 1, 2),
    # ---- tta_patches_kernel: octets against hash calls
    "tta: NO == HQ": (lambda c: TTA in c.kernels and W.octets(c.C) == W.hash_calls(c.C), 2),
    "tta: NO < HQ": (lambda c: TTA in c.kernels and W.octets(c.C) < W.hash_calls(c.C), 2),
    "tta: C % 8 != 0 (the b < C guards)": (lambda c: TTA in c.kernels and c.C % 8 != 0, 2),
    # ---- the mirror at its limits
    "mirror: rows = cols = w / 2": (lambda c: c.scene == "half" and EXTRACT in c.kernels and TTA in c.kernels, 3),
    "mirror: rows = cols = w (the feed's smallest scene)": (lambda c: c.scene == "exact" and FEED in c.kernels, 3),
    "mirror: cols = w - 1, no interior column": (lambda c: c.scene == "narrow" and EXTRACT in c.kernels, 3),
}
# the off-by-one places: ONE (C, w) each is what the table must hold (for each kernel)
EDGES_C = (64, 65, 128, 129, 192, 193, 255, 256)
EDGES_TTA = (7, 8, 9, 15, 16, 17, 255, 256)
FEED_PER8 = range(8)
# the (C, w) the table was asked to hold, whatever else it holds
REQUIRED = [(1, 4), (2, 5), (3, 5), (5, 6), (6, 7), (64, 8), (65, 8), (128, 8), (129, 9), (192, 8), (193, 8), (255, 12),
            (256, 12), (101, 20), (100, 20), (1, 1), (2, 1), (3, 1), (1, 2), (1, 3)]


@pytest.mark.parametrize("name", list(REGIMES), ids=list(REGIMES))
def test_every_regime_is_covered(name):
    pred, least = REGIMES[name]
    hits = [c.id for c in CASES if pred(c)]
    print("%s: %s" % (name, ", ".join(hits)))                     # (the regime -> cases listing, under -s)
    assert len(hits) >= least, (name, hits)


def test_the_off_by_one_channel_counts_are_in_the_table():
    for ch in EDGES_C:
        for k in (EXTRACT, FEED, TTA):
            assert any(c.C == ch and k in c.kernels for c in MARGIN), (ch, k)
    for ch in EDGES_TTA:
        assert any(c.C == ch and TTA in c.kernels for c in MARGIN), ch
    for r in FEED_PER8:                       # every residue of the row length against the feed's eight-element store
        assert any(FEED in c.kernels and c.values()["per8"] == r for c in CASES), r
    # the C limit and the largest window admit one (C, w) each
    assert sum(c.C == 256 for c in MARGIN) == 1 and sum(c.w == 20 and c.C & 1 for c in MARGIN) == 1


def test_deleting_any_one_case_is_noticed():
    """the coverage assertions above fail for the table less any one of its cases"""
    def covered(cases):
        margin = [c for c in cases if c.scene == "margin"]
        if not {(c.C, c.w) for c in margin} >= set(REQUIRED):
            return False
        if not all(sum(bool(p(c)) for c in cases) >= n for p, n in REGIMES.values()):
            return False
        if not all(any(c.C == ch and k in c.kernels for c in margin) for ch in EDGES_C for k in (EXTRACT, FEED, TTA)):
            return False
        if not all(any(c.C == ch and TTA in c.kernels for c in margin) for ch in EDGES_TTA):
            return False
        return all(any(FEED in c.kernels and c.values()["per8"] == r for c in cases) for r in FEED_PER8)
    assert covered(CASES)
    slack = [c.id for c in CASES if covered([d for d in CASES if d is not c])]
    assert slack == [], slack


def test_the_required_pairs_are_in_the_table():
    have = {(c.C, c.w) for c in MARGIN}
    assert not [p for p in REQUIRED if p not in have]
    v = W.BY_ID["c255-w12"].values()
    assert W.items(255, 12) == 9180 and v["batches"] == 3
    assert W.items(256, 12) == 9216 and W.BY_ID["c256-w12"].values()["tile_lds"] == 148032
    assert W.items(101, 20) == 10100 and W.BY_ID["c101-w20"].values()["extract_lds"] == 161600
    assert [W.rem(*p) for p in ((1, 4), (2, 5), (3, 5), (5, 6), (6, 7), (129, 9))] == [0, 2, 3, 2, 2, 1]
    for c in MARGIN:
        assert c.rows != c.cols and c.rows > c.w and c.cols > c.w and c.rows * c.cols <= 600, c.id
        n = len(W.pixel_list(c))
        assert n == c.rows * c.cols or c.w == 20
        assert n * W.per(c.C, c.w) * 4 < 40 << 20, c.id           # the largest output: tens of MB
    for c in CASES:
        if c.w == 20:                                             # both outer rings whole, and a dozen inside
            pix = W.pixel_list(c)
            r, q = pix // c.cols, pix % c.cols
            ring = (r < 2) | (r >= c.rows - 2) | (q < 2) | (q >= c.cols - 2)
            assert ring.sum() == c.rows * c.cols - (c.rows - 4) * (c.cols - 4) and (~ring).sum() == 12


# ------------------------------------------------------------------ 2. the float-reciprocal quotients
def _quotient(t, d):
    """(int)(((float)t + 0.5f) * (1.0f / (float)d)) in float32, as the kernels form it"""
    inv = np.float32(1.0) / np.float32(d)
    return ((t.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


def test_the_reciprocal_quotients_are_the_integer_quotients_over_the_envelope():
    shapes = 0
    seen_n4 = set()
    for w in range(1, 21):
        for C in range(1, 257):
            if W.extract_lds(C, w) > LDS_MAX:
                continue
            shapes += 1
            q4, NI, NF = W.n4(C, w), W.items(C, w), w * C
            if q4 > 0 and (q4, w) not in seen_n4:                 # (the row of an item depends on n4 and w alone)
                seen_n4.add((q4, w))
                t = np.arange(NI, dtype=np.int64)
                assert np.array_equal(_quotient(t, q4), t // q4), (C, w, "item -> row")
            e0 = np.arange(NF, dtype=np.int64)
            assert np.array_equal(_quotient(e0, C), e0 // C), (C, w, "element -> pixel")
    assert shapes > 4000                                          # (most of 20 x 256: the envelope is what was walked)
    for C, w in ((256, 13), (102, 20), (103, 20)):
        assert W.extract_lds(C, w) > LDS_MAX or W.tile_lds(C, w) > LDS_MAX


# ------------------------------------------------------------------ 3. the reference is not a transposed g
def _scene_under(S, g):
    """the scene whose pixel (i, j) is S's pixel under element g (``spatial_index`` on a rows x cols grid)"""
    R, Q = S.shape[:2]
    T = np.swapaxes(S, 0, 1) if g & 4 else S                      # T[i][j] = S[a][b], (a, b) = (j, i) or (i, j)
    # the flips are of S's own axes: a is S's row (flipped by g & 2), b its column (flipped by g & 1)
    if g & 4:
        T = T[:, ::-1] if g & 2 else T
        T = T[::-1, :] if g & 1 else T
    else:
        T = T[::-1, :] if g & 2 else T
        T = T[:, ::-1] if g & 1 else T
    return np.ascontiguousarray(T)


def _pixel_under(r, c, R, Q, g):
    """where S's pixel (r, c) sits in ``_scene_under(S, g)``, and that scene's column count"""
    a = R - 1 - r if g & 2 else r
    b = Q - 1 - c if g & 1 else c
    return ((b, a), R) if g & 4 else ((a, b), Q)


@pytest.mark.parametrize("g", range(8))
def test_the_spatial_reference_is_the_cut_of_the_transformed_scene(g):
    case = W.BY_ID["c3-w5"]                                        # an odd window: the identity holds for every element
    S, w = W.cube_of(case), case.w
    assert w & 1
    pix = W.pixel_list(case)
    want = W.apply_elements(W.cut_of(case), g)
    Sg = _scene_under(S, g)
    mapped = []
    for P in pix:
        (i, j), cols_g = _pixel_under(int(P) // case.cols, int(P) % case.cols, case.rows, case.cols, g)
        mapped.append(i * cols_g + j)
    got = O.extract_patches(Sg, w, np.array(mapped))
    assert np.array_equal(got, want)
    if g:                                                          # and the elements are not each other
        assert not np.array_equal(want, W.cut_of(case))


def test_the_noise_helpers_are_the_documented_counters():
    """row i of a batch: stream 0x100 + net over pairs of 16-byte groups for the patches, 0x200 + net over groups for the
    spectra, counter (global sample << 24) | index -- the statement of tests/test_gpu_step.py"""
    from tests.test_noise_generator_math import _ctr, noise_normal4, noise_normal8
    z = W.training_patch_noise(1088, 0, 1, 17, 3, 5)
    assert z.shape == (75,) and z.dtype == np.float32
    assert np.array_equal(z, noise_normal8(1088, 0, 0x101, _ctr(17, np.arange(10))).T.reshape(-1)[:75])
    s = W.training_spectrum_noise(1088, 0, 0, 17, 7)
    assert np.array_equal(s, noise_normal4(1088, 0, 0x200, _ctr(17, np.arange(2))).T.reshape(-1)[:7])
    assert W.global_samples(12, 12).tolist() == list(range(24))


# ------------------------------------------------------------------ 4. every case is a shape its kernel accepts
def test_every_case_is_a_shape_its_kernels_accept():
    from cmlpl_amd import _lib
    lib = _lib.load()
    for c in CASES:
        fit = lib.cmlpl_patches_fit(c.C, c.w)
        v = c.values()
        if EXTRACT in c.kernels:
            assert fit & 1 and v["extract_lds"] <= LDS_MAX and c.rows >= c.w // 2 and c.cols >= c.w // 2, c.id
        if TTA in c.kernels:
            assert fit & 2 and v["tile_lds"] <= LDS_MAX and c.rows >= c.w // 2 and c.cols >= c.w // 2, c.id
        if FEED in c.kernels:                                     # make_dims' window, the step's scene, the feed's tile
            assert 4 <= c.w <= 20 and 1 <= c.C <= 256 and c.rows >= c.w and c.cols >= c.w and v["tile_lds"] <= LDS_MAX, c.id
    for C, w in W.FEED_REFUSED:
        assert W.tile_lds(C, w) > LDS_MAX and 4 <= w <= 20 and C <= 256
    assert lib.cmlpl_patches_fit(*W.CUT_REFUSED) == 0
    for name in W.AUGMENT_CASES + W.FEED_BY_INDEX + W.FEED_SPATIAL + W.FEED_VS_SPLIT + [W.DEALING_CASE, W.FEED_BANDS300]:
        assert name in W.BY_ID
    pers = [W.per(W.BY_ID[n].C, W.BY_ID[n].w) for n in W.AUGMENT_CASES]
    assert sum(p % 4 == 0 for p in pers) >= 2 and sum(p % 4 != 0 for p in pers) >= 2
    sp = [W.BY_ID[n] for n in W.FEED_SPATIAL]
    assert any(c.values()["per8"] for c in sp) and any(c.C > 128 for c in sp)
    assert all(FEED in W.BY_ID[n].kernels for n in W.FEED_BY_INDEX + W.FEED_SPATIAL + W.FEED_VS_SPLIT + [W.FEED_BANDS300])
