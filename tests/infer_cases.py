"""The inference-envelope table: one case per regime of whole-scene prediction (cmlpl_infer_cube / cmlpl_infer_pixels and
their views; by patches: cmlpl_extract_patches + cmlpl_basenet2_fwd).  Plain data (no device, no library):
tests/test_gpu_infer_envelope.py runs the cases on the GPU against the fp64 oracle, tests/test_infer_route_cpu.py holds
the library's routing answers (infer_fused, infer_supported) to the same table without one.

What the regimes are (conv3_stage's CUBE branches in csrc/conv3x3.hip): the window is gathered from the band-last cube in
CHUNKS of 16 bands, KQ0 = ceil(C / 16) of them; a pass holds SLAB_RING = 7 chunks with SLAB_WIN = 4 in flight, so KQ0 >= 5
refills the in-flight window, C = 113 starts a second pass with one band and C > 224 a third.  Windows of 8 .. 11 run
the four-wave kernels ("fused4"), windows of 12 .. 15 the eight-tile ones ("fused8"); every other window -- smaller than
8, 16 and larger -- is cut on the device and goes through the general forward ("patches"), as long as one window fits
the cut's LDS (cmlpl_patches_fit: 101 channels at 20 x 20).  The launcher's limit on the scene is rows, cols >= w / 2
(one mirror fold): the "tiny" cases sit on it."""
from typing import NamedTuple

FUSED4, FUSED8, PATCHES = "fused4", "fused8", "patches"


class Case(NamedTuple):
    id: str
    shape: tuple        # (C, w, w, bands, K)
    rows: int           # the scene
    cols: int
    route: str          # FUSED4: four-wave fused kernel, FUSED8: eight-tile fused kernel, PATCHES: cut + general forward
    why: str

    @property
    def fused(self):
        return self.route != PATCHES


CASES = [
    Case("f4-min", (1, 8, 8, 1, 1), 10, 11, FUSED4, "one band, one class, HW = 64 (one 16-byte item per lane pair)"),
    Case("f4-w9", (17, 9, 9, 5, 17), 11, 12, FUSED4, "window 9; second chunk of one band; second class chunk of one class"),
    Case("f4-c80", (80, 8, 8, 3, 2), 10, 11, FUSED4, "KQ0 = 5: the first refill of the in-flight window"),
    Case("f4-c112", (112, 11, 11, 9, 16), 13, 14, FUSED4, "exactly one full pass; K = 16 exactly"),
    Case("f4-c113", (113, 10, 10, 300, 33), 12, 13, FUSED4, "second pass of one band; more than 256 spectral bands; K = 33"),
    Case("f4-c256", (256, 11, 11, 16, 64), 13, 14, FUSED4, "three passes; four full class chunks"),
    Case("f8-w13", (3, 13, 13, 2, 2), 15, 16, FUSED8, "window 13; fewer bands than a quad"),
    Case("f8-c112", (112, 12, 12, 8, 32), 14, 15, FUSED8, "one full pass on eight waves"),
    Case("f8-c113", (113, 15, 15, 7, 49), 17, 18, FUSED8, "second pass on eight waves; K = 49"),
    Case("f8-c225", (225, 13, 13, 4, 48), 15, 16, FUSED8, "third pass of one band"),
    Case("f8-c256", (256, 14, 14, 11, 64), 16, 17, FUSED8, "the largest accepted"),
    Case("p-w4", (5, 4, 4, 6, 3), 6, 7, PATCHES, "the smallest window (P4 = 1)"),
    Case("p-w7", (33, 7, 7, 9, 10), 9, 10, PATCHES, "just under the fused windows"),
    Case("p-w16", (20, 16, 16, 5, 4), 18, 19, PATCHES, "256 pixels but P4 = 16: the fused kernels' boundary"),
    Case("p-w20", (101, 20, 20, 12, 9), 22, 12, PATCHES,
         "the most channels the cut takes at 20 x 20; scene narrower than the window"),
    Case("tiny-11", (103, 11, 11, 103, 9), 5, 5, FUSED4, "scene = W/2 both ways: every window folds on all four sides"),
    Case("tiny-15", (48, 15, 15, 48, 20), 7, 30, FUSED8, "rows = W/2 only"),
    Case("tiny-8", (30, 8, 8, 30, 5), 40, 4, FUSED4, "cols = W/2 only, even window"),
]
BY_ID = {c.id: c for c in CASES}

# Windows no cut takes (one window past 160 KiB of LDS): infer_supported must say no, infer_cube must refuse before a launch.
# Raw PaviaU bands under the reference's own 20 x 20 window, and the first even / odd channel counts past the limit there.
CUT_TOO_LARGE = [(103, 20, 20, 103, 9), (102, 20, 20, 5, 3), (256, 16, 16, 4, 2)]
# ... and what still fits next to them (p-w20 is the table's own): the reference's 20 x 20 x 60, the limit at 16 x 16
CUT_FITS = [(60, 20, 20, 103, 9), (101, 20, 20, 12, 9), (159, 16, 16, 4, 2), (255, 4, 4, 4, 2)]
# the cases that run again by patches under CMLPL_FUSE_TAIL=0, and the one whose window no cut takes then
FORCED_BY_PATCHES = ("f4-c256", "f8-c112")
FORCED_REFUSED = "f8-c256"
# The views of test-time augmentation are held to the oracle on the tensors `views_of` returns, and `views_of` is the view
# cut: it takes f4-c256 (124 KB) and f8-c113 (102 KB) but not 256 channels at 14 x 14 (201 KB).  f8-c225 (152 KB) is the
# three-pass eight-tile case whose views exist as tensors; f8-c256 keeps what needs none (VIEW_NO_CUT: the pure spatial
# element, built on the host from its definition, and the noisy view's independence of the feed).
VIEW_CASES = ("f4-c256", "f8-c113", "f8-c225")
VIEW_NO_CUT = "f8-c256"
ARGMAX_CASES = ("f4-c112", "p-w7")
