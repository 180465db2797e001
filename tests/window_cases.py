"""The window-gather table: one case per regime of the three kernels that cut a w x w x C window out of the resident scene
cube with the symmetric, edge-repeating mirror -- extract_patches_kernel (csrc/augment.hip, behind cmlpl_extract_patches),
cube_feed_kernel (csrc/cube_feed.hip, the patch source of every cube-fed training step) and tta_patches_kernel
(csrc/tta.hip, behind cmlpl_tta_patches_sym / ``views_of``) -- and the HOST reference they are held to.  Plain data and
numpy (no device, no library): tests/test_gpu_window_envelope.py runs the cases on the GPU, tests/test_window_cases_cpu.py
holds the table itself (every regime named below is hit, the kernels' float-reciprocal index arithmetic is exact over the
whole envelope, the reference is not transposed) without one.

The reference adds no arithmetic of its own: the clean window is ``oracle.cmlpl_oracle.extract_patches``, a spatial
element is ``tests.test_spatial_host.spatial_index`` gathered from that cut, a training row's element is
``training_elements``, the training noise is ``noise_normal8`` / ``noise_normal4`` of tests/test_noise_generator_math.py
under the counters tests/test_gpu_step.py documents, a view's noise is ``view_window_noise`` of tests/test_tta_host.py.

The regime functions restate the kernels' inline arithmetic:
  extract_patches_kernel / cube_feed_kernel, a window OFF the column margin: w spans of NF = w C consecutive floats, each
  n4 = NF >> 2 16-byte items and rem = NF & 3 floats behind them; NI = w n4 items per window, 4096 per batch (512 threads,
  eight in flight).  extract_patches_kernel keeps two LDS layouts (odd C: row stride NF rounded up to 4, aligned 16-byte
  LDS writes; even C: pixel stride C + 1, element by element).  A window ON the column margin: a wave per pixel, lanes =
  channels, 128 per pass in two halves of 64.  The scatter of extract_patches_kernel walks 256 window pixels at a time,
  a wave per band (eight waves); cube_feed_kernel stores eight consecutive elements per thread, 16 bytes at a time while
  all eight are inside the row (per = C w w).  tta_patches_kernel's item is a band octet of a window pixel (NO = ceil(C / 8)
  per pixel) and its noise counter advances HQ = 2 ceil(C / 16) per pixel."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np

from oracle import cmlpl_oracle as O
from tests.test_noise_generator_math import _ctr, noise_normal4, noise_normal8
from tests.test_spatial_host import spatial_index, training_elements
from tests.test_tta_host import view_window_noise

LDS_MAX = 160 * 1024
EXTRACT, FEED, TTA = "extract", "feed", "tta"
ALL = (EXTRACT, FEED, TTA)
CUTS = (EXTRACT, TTA)
NOISE_TOL = 2e-5                # the project's allowance for the hardware's log2 / sin / cos (tests/test_gpu_step.py)
STREAM_NOISE_XP, STREAM_NOISE_X = 0x100, 0x200


# ------------------------------------------------------------------ the kernels' arithmetic, restated
def layout(C):
    return "odd" if C & 1 else "even"


def nf(C, w):
    return w * C


def n4(C, w):
    return (w * C) >> 2


def rem(C, w):
    return (w * C) & 3


def items(C, w):
    return w * n4(C, w)


def batches(C, w):
    """batches of 4096 16-byte items a window off the column margin takes (0: n4 == 0, the spans are all tail)"""
    return -(-items(C, w) // 4096)


def passes(C):
    """128-channel passes of the column-margin path"""
    return -(-C // 128)


def second_half_live(C):
    """the second half (lanes 64 .. 127) of the LAST pass carries channels"""
    return (C - 1) % 128 >= 64


def big_window(w):
    return w * w > 256


def per(C, w):
    return C * w * w


def extract_lds(C, w):
    rs = ((w * C + 3) & ~3) if C & 1 else w * (C + 1)
    return w * rs * 4


def tile_lds(C, w):
    """cube_feed_kernel's and tta_patches_kernel's tile"""
    return w * w * (C | 1) * 4


def octets(C):
    return (C + 7) >> 3


def hash_calls(C):
    return 2 * ((C + 15) >> 4)


# ------------------------------------------------------------------ the table
class Case(NamedTuple):
    id: str
    C: int
    w: int
    rows: int
    cols: int
    kernels: tuple      # which of EXTRACT / FEED / TTA the case is for
    scene: str          # "margin": a few pixels larger than the window; "half" / "exact" / "narrow": the limit scenes
    why: str

    def values(self):
        C, w = self.C, self.w
        return dict(layout=layout(C), rem=rem(C, w), n4=n4(C, w), batches=batches(C, w), passes=passes(C),
                    second_half=second_half_live(C), big=big_window(w), per8=per(C, w) % 8,
                    extract_lds=extract_lds(C, w), tile_lds=tile_lds(C, w))


def _margin(C, w, kernels, why):
    return Case("c%d-w%d" % (C, w), C, w, w + 3, w + 2, kernels, "margin", why)


_SHAPES = [
    # (C, w), kernels, why
    ((1, 4), ALL, "C < 4, odd layout, rem 0: four pixels per 16-byte item; the smallest window the feed takes"),
    ((2, 5), ALL, "C < 4, even layout, rem 2: the ++ch == C wrap fires twice per item"),
    ((3, 5), ALL, "C < 4, odd layout, rem 3"),
    ((2, 7), ALL, "C < 4, even layout again (rem 2), odd window"),
    ((5, 5), ALL, "per % 8 == 5; rem 1"),
    ((5, 6), ALL, "odd C, rem 2"),
    ((6, 7), ALL, "even C, rem 2"),
    ((7, 5), ALL, "octets: C = 8 - 1; rem 3; per % 8 == 7"),
    ((8, 5), CUTS, "octets: C = 8 exactly, NO = 1 against HQ = 2"),
    ((9, 5), ALL, "octets: C = 8 + 1; per % 8 == 1"),
    ((15, 5), CUTS, "octets: C = 16 - 1; rem 3"),
    ((16, 5), CUTS, "octets: C = 16 exactly, NO = HQ = 2"),
    ((17, 5), CUTS, "octets: C = 16 + 1, HQ = 4 against NO = 3"),
    ((3, 17), ALL, "w * w = 289 > 256 with odd C: the scatter's second walk; rem 3; waves without a band"),
    ((64, 8), ALL, "margin path: exactly the first half of a pass"),
    ((65, 8), ALL, "margin path: one channel in the second half"),
    ((128, 8), ALL, "margin path: exactly one pass"),
    ((129, 9), ALL, "margin path: one channel in the second pass; rem 1; per % 8 == 1"),
    ((192, 8), ALL, "margin path: exactly three halves"),
    ((193, 8), ALL, "margin path: one channel in the last half"),
    ((255, 12), ALL, "odd C, NI = 9180: three batches in the odd layout; margin channels above 192; C = 256 - 1"),
    ((256, 12), ALL, "even C, NI = 9216; the C limit; 148,032 bytes of LDS"),
    ((101, 20), ALL, "the largest window: NI = 10100 in the odd layout, w * w = 400; 161,600 of 163,840 bytes of LDS"),
    ((100, 20), ALL, "the same, even C"),
    ((1, 1), (EXTRACT,), "n4 == 0: a one-float span"),
    ((2, 1), (EXTRACT,), "n4 == 0, even layout"),
    ((3, 1), (EXTRACT,), "n4 == 0, rem 3"),
    ((1, 2), (EXTRACT,), "n4 == 0, two pixels per span"),
    ((1, 3), (EXTRACT,), "n4 == 0, rem 3 over three pixels"),
]
# the limit scenes, for one odd window with C < 4, one even window and one C > 128
_LIMITS = [(3, 5), (5, 6), (129, 9)]


def _limit(C, w, scene):
    if scene == "half":
        return Case("c%d-w%d-half" % (C, w), C, w, w // 2, w // 2, CUTS, scene,
                    "rows = cols = w / 2: the single fold lands exactly on the far edge")
    if scene == "exact":
        return Case("c%d-w%d-exact" % (C, w), C, w, w, w, ALL, scene,
                    "rows = cols = w: the smallest scene the cube-fed step takes, one interior column")
    return Case("c%d-w%d-narrow" % (C, w), C, w, w + 3, w - 1, CUTS, scene,
                "cols = w - 1: no interior column, every window goes pixel by pixel (the engine refuses cols < w)")


CASES = [_margin(C, w, k, why) for (C, w), k, why in _SHAPES] + \
        [_limit(C, w, s) for C, w in _LIMITS for s in ("half", "exact", "narrow")]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# shapes the feed must refuse (its tile past 160 KiB): the first even C past the limit at 20 x 20, the C limit at 13 x 13
FEED_REFUSED = [(102, 20), (256, 13)]
# a window no cut takes, for the refusal of cmlpl_extract_patches
CUT_REFUSED = (103, 20)
# cmlpl_augment, called directly: the patch rows of six table cases (per % 4 == 0 and != 0), spectra rows of these lengths
AUGMENT_CASES = ["c1-w4", "c3-w5", "c5-w6", "c9-w5", "c65-w8", "c129-w9"]
AUGMENT_BANDS = [1, 3, 4, 7, 300, 1028, 1029]
# the extra list lengths of the dealing check (p = (b & 7) ceil(n / 8) + (b >> 3)), over a prefix of one case's pixel list
DEALING_CASE, DEALING_LENGTHS = "c5-w6", (1, 2, 7, 8, 9, 15)
# cube-fed extras
FEED_BANDS300 = "c5-w6"                                  # bands = 300: the unfused spectral launch is in play
FEED_BY_INDEX = ["c3-w5", "c65-w8"]
FEED_SPATIAL = ["c3-w5", "c6-w7", "c129-w9"]              # per % 8 == 3 and 6, and C > 128
FEED_VS_SPLIT = ["c2-w5", "c193-w8"]                     # the split-fed step on the ORACLE's windows


def cases_for(kernel):
    return [c for c in CASES if kernel in c.kernels]


# ------------------------------------------------------------------ scenes, pixel lists, the reference
def _seed(case):
    return 1000 * case.C + 10 * case.w + len(case.scene)


@lru_cache(maxsize=None)
def cube_of(case):
    """the scene: seeded standard normals, float32 (as tests/test_patches.py)"""
    c = np.random.Generator(np.random.PCG64(_seed(case))).standard_normal((case.rows, case.cols, case.C)).astype(np.float32)
    c.setflags(write=False)
    return c


def pixel_list(case):
    """EVERY pixel of the scene in raster order (every kind of mirrored border, and the interior); for w = 20 the two outer
    rings and a dozen interior pixels, which keeps the largest output in the tens of MB"""
    rows, cols = case.rows, case.cols
    every = np.arange(rows * cols, dtype=np.int64)
    if case.w < 20:
        return every
    r, c = every // cols, every % cols
    ring = (r < 2) | (r >= rows - 2) | (c < 2) | (c >= cols - 2)
    inner = every[~ring]
    pick = inner[np.linspace(0, len(inner) - 1, 12).astype(np.int64)]
    return np.sort(np.concatenate([every[ring], pick]))


@lru_cache(maxsize=None)
def cut_of(case):
    """the oracle's windows of ``pixel_list(case)``: [n, C, w, w], computed once and read-only"""
    out = O.extract_patches(cube_of(case), case.w, pixel_list(case))
    out.setflags(write=False)
    return out


def cut(case, pix):
    """the oracle's windows of any pixels of the case's scene"""
    return O.extract_patches(cube_of(case), case.w, np.asarray(pix, dtype=np.int64))


def apply_elements(win, g):
    """windows [n, C, w, w] with row s under spatial element g[s] (an int: all rows): output pixel p shows window pixel
    spatial_index(g, w)[p]"""
    n, C, w, _ = win.shape
    g = np.broadcast_to(np.asarray(g, dtype=np.int64), (n,))
    flat = win.reshape(n, C, w * w)
    out = np.empty_like(flat)
    for s in range(n):
        out[s] = flat[s][:, spatial_index(int(g[s]), w)]
    return out.reshape(win.shape)


def training_patch_noise(seed, step, net, sample, C, w):
    """N(0,1) of one training patch row [C w w]: stream 0x100 + net, counter (global sample << 24) | pair of 16-byte groups"""
    p = per(C, w)
    return noise_normal8(seed, step, STREAM_NOISE_XP + net, _ctr(sample, np.arange((p + 7) // 8))).T.reshape(-1)[:p]


def training_spectrum_noise(seed, step, net, sample, bands):
    return noise_normal4(seed, step, STREAM_NOISE_X + net, _ctr(sample, np.arange((bands + 3) // 4))).T.reshape(-1)[:bands]


def global_samples(bt, btu):
    """the global sample of batch row s: labelled row i is i, unlabelled row i is bt + i"""
    return np.arange(bt + btu)


__all__ = ["Case", "CASES", "BY_ID", "cases_for", "cube_of", "pixel_list", "cut_of", "cut", "apply_elements",
           "training_patch_noise", "training_spectrum_noise", "training_elements", "view_window_noise", "global_samples"]
