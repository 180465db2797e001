"""The two-piece range table: one case per kernel family that has a loop on TWO fp16 pieces, with
the router's answer for it (cmlpl_debug_route / cmlpl_debug_two_piece: host arithmetic, asked before anything runs, as
tests/envelope_cases.py does for the regimes), and the exponents the range tests place their images at.  Plain data: no
device.  tests/test_f16x2_bound_cpu.py walks the table on the CPU, tests/test_gpu_f16x2_range.py on the GPU."""
from typing import NamedTuple


class Case(NamedTuple):
    name: str
    shape: tuple        # (C, H, W, bands, K)
    nets: int
    n: int              # rows the router is asked about (and every row count a test of this file's cases runs: ROWS)
    fwd: str            # regimes
    bwd: str
    big: bool           # the eight-tile per-sample kernels
    fwd_ps: tuple       # per-sample forward / backward launch: (waves, tiles per wave, 1 = conv1's loop on two pieces)
    bwd_ps: tuple
    h2x: tuple          # the four general plans (conv1 fwd, conv1 dgrad, conv2 fwd, conv2 dgrad): 1 = two pieces
    stats: int          # the per-sample maxima table is written (the weight gradients can take two-piece planes)
    two_piece: int      # cmlpl_debug_two_piece: bit 0 conv1 fwd, 1 conv1 dgrad, 2 weight gradients, 3 conv2 fwd + dgrad
    why: str

    @property
    def id(self):
        return self.name + "-" + "x".join(map(str, self.shape))

    @property
    def conv2_two_piece(self):
        """conv2's tap loops run as launches of their own on two pieces (the fused tail / head are three-piece)"""
        return bool(self.two_piece & 8)

    @property
    def da0_in_hbm(self):
        """the general backward writes da0; the fused backward A keeps it on chip (read through conv0's weight gradient)"""
        return self.bwd == "C"


ROWS = (4, 8, 10, 12, 16)          # every batch size the range tests use: the route must not depend on it
CASES = [
    Case("ks8", (103, 11, 11, 5, 3), 1, 8, "A", "A", False, (8, 1, 1), (8, 1, 1), (1, 1, 0, 0), 1, 7,
         "per-sample kernels, four tiles, eight waves; below C ~ 103 at 11 x 11 the backward is regime B (no two-piece loop)"),
    Case("big", (4, 12, 12, 4, 3), 1, 4, "A", "A", True, (8, 2, 1), (8, 2, 1), (0, 0, 1, 1), 1, 7,
         "per-sample kernels, eight tiles (conv2 runs in their fused tail / head: three pieces)"),
    Case("gen16", (4, 16, 16, 4, 3), 1, 4, "C", "C", False, (0, 0, 0), (0, 0, 0), (1, 1, 1, 1), 1, 15,
         "general path, one sample per workgroup, eight waves, one tile per wave; conv2 on the barrier-free loop"),
    Case("gen17", (4, 17, 17, 4, 3), 1, 4, "C", "C", False, (0, 0, 0), (0, 0, 0), (1, 1, 1, 1), 1, 15,
         "general path, odd window: two tiles per wave in the data gradient, a last row and column the pool drops"),
]

# the four-wave, four-tile per-sample kernels appear with two networks and many rows only: the smallest row count per
# network at which the router picks them (asserted: one row fewer still gets eight waves)
FOUR_WAVE = {"shape": (103, 11, 11, 5, 3), "nets": 2, "n": 129, "ps": (4, 2, 1)}

EDGE_EXPONENTS = (39, 40, 41, 127, 199, 200, 201)       # exponent fields of the image maxima of ONE batch
WGRAD_CORNERS = ((40, 120), (120, 40), (200, 40), (40, 200), (100, 60), (100, 59), (39, 127), (127, 201))   # (ea, eg)


def route(shape, nets, n):
    """the router's answer as a dict (needs the built library, no device)"""
    import ctypes as C
    from cmlpl_amd import _lib
    lib = _lib.load()
    out = (C.c_int * 30)()
    cs = _lib.Shape(*shape)
    _lib.check("cmlpl_debug_route", lib.cmlpl_debug_route(C.byref(cs), nets, n, out))
    o = list(out)
    return {"fwd": "ABC"[o[0]], "bwd": "ABC"[o[1]], "big": bool(o[2]), "fwd_ps": tuple(o[3:6]), "bwd_ps": tuple(o[6:9]),
            "h2x": tuple(o[13 + 5 * i] for i in range(4)), "stats": o[29],
            "two_piece": lib.cmlpl_debug_two_piece(C.byref(cs), nets, n)}


def assert_route(case, rows=None):
    """the case runs what the table says, at every row count the tests use (under the default switches)"""
    want = {k: getattr(case, k) for k in ("fwd", "bwd", "big", "fwd_ps", "bwd_ps", "h2x", "stats", "two_piece")}
    for n in sorted(set((case.n,) + tuple(rows or ROWS))):
        got = route(case.shape, case.nets, n)
        assert got == want, (case.id, n, got, want)
