"""The weight-gradient regime table: one case per regime of the 3x3 weight-gradient kernels (csrc/wgrad3x3.hip), and what
the CMLPL_WGRAD3_* switches make of each.  Plain data and arithmetic plus a reader of the library's own plan
(cmlpl_debug_wgrad3_plan: host arithmetic, no device): tests/test_gpu_wgrad_envelope.py runs the cases on the GPU
against the fp64 oracle, tests/test_wgrad_plan_cpu.py holds the planner to the same table without one.

All cases run through BaseNet2 (one network).  The row counts are the smallest that give the regime on 256 compute
units (a single launch spreads a map over 256 / 3 = 85 workgroups per kernel row, a pair launch over 64 + 21); a device
with fewer units makes MORE stages per workgroup, so the stage counts are lower limits."""
import ctypes as C
import os
from typing import NamedTuple

PAIRS = ((4, 2), (5, 2), (6, 3), (7, 3), (8, 4), (9, 4), (10, 5))     # wgrad3b_pair_kernel<CA, CB> as instantiated
MAXCPR = 11                                                          # wgrad3b_kernel<CPR>: 1 .. 11
LDS_MAX = 160 * 1024


def wg3b_U(cpr):
    """pooled rows per stage of wgrad3b_kernel<cpr> (wgrad3x3.hip: wg3b_U)"""
    return min(97 // (4 * cpr + 3), 32 // cpr, 16) & ~1


def geometry(U, UPS):
    """how a stage of U pooled rows lies against samples of UPS pooled rows: the constants of the carried-offset advance
    (qU = U / UPS, rU = U % UPS) change character between these four"""
    return "lt" if U < UPS else "eq" if U == UPS else "mult" if U % UPS == 0 else "rem"


class MapPlan(NamedTuple):
    cpr: int; b3: int; U: int; UPG: int; G: int; lds: int; cspl: int

    @property
    def stages(self):
        return self.UPG // self.U if self.cpr else 0


class Plan(NamedTuple):
    maps: tuple         # (MapPlan of the window, MapPlan of its pooled map)
    pair: bool
    slist: bool         # the pair launch would place the zero-skip sample list
    cus: int


def read_plan(shape, nets, n):
    from cmlpl_amd import _lib
    out = (C.c_int * 17)()
    _lib.check("cmlpl_debug_wgrad3_plan", _lib.load().cmlpl_debug_wgrad3_plan(C.byref(_lib.Shape(*shape)), nets, n, out))
    o = list(out)
    return Plan((MapPlan(*o[0:7]), MapPlan(*o[7:14])), bool(o[14]), bool(o[15]), o[16])


class Case(NamedTuple):
    tag: str            # "stage": several stages per workgroup under the default switches; "few": run under CMLPL_WGRAD3_RG;
                        # "general": a window too wide for the row-split kernels; "skip": the compacted body
    shape: tuple        # (C, H, W, bands, K)
    n: int
    cpr: tuple          # column pairs per row of the two maps (0: the general kernel) under the default switches
    pair: bool          # one launch for both maps under the default switches
    stages: tuple       # stages per workgroup of the two maps on 256 compute units, default switches (lower limits)
    geo: tuple          # geometry(U, UPS) of the two maps ("-": the general kernel)
    two: bool           # the step leaves the maxima table (in a pair launch the two-piece body runs and the list is placed)
    why: str
    skip: tuple = ()    # patterns of zeroed upstream-gradient rows the compacted body is run with ("alternate", "all-but-one", "third")
    poison: bool = False  # also run with a non-finite activation in a zero-gradient sample

    @property
    def id(self):
        return f"{self.tag}-cpr{self.cpr[0]}_{self.cpr[1]}-" + "x".join(map(str, self.shape[:3])) + f"-n{self.n}"


def _c(tag, chw, n, cpr, pair, stages, geo, two, why, skip=(), poison=False):
    return Case(tag, tuple(chw) + (4, 3), n, cpr, pair, stages, geo, two, why, skip, poison)


CASES = [
    # several stages per workgroup: the double-buffered hand-off and the carried-offset advance, per kernel
    _c("stage", (3, 4, 4), 1021, (2, 1), False, (4, 2), ("mult", "mult"), False, "CPR 1 with two stages (2 x 2 map, one pooled row per sample), CPR 2 with four"),
    _c("stage", (3, 6, 6), 171, (3, 1), False, (2, 1), ("mult", "mult"), False, "CPR 3 as the first map, U = 2 UPS"),
    _c("stage", (3, 16, 6), 64, (3, 1), False, (2, 1), ("lt", "mult"), False, "CPR 3, H > W: the wrap inside a sample (U = 6 < UPS = 8)"),
    _c("stage", (3, 20, 4), 205, (2, 1), False, (4, 2), ("lt", "rem"), False, "H > W: CPR 2 with UPS = 10, CPR 1 with U = 12 over UPS = 5 (qU = 2, rU = 2)"),
    _c("stage", (3, 8, 8), 86, (4, 2), True, (2, 2), ("eq", "mult"), False, "pair (4, 2), U = UPS for the first map"),
    _c("stage", (3, 6, 8), 169, (4, 2), True, (2, 2), ("rem", "mult"), False, "pair (4, 2) with U = 4 over UPS = 3 (qU = 1, rU = 1)"),
    _c("stage", (3, 7, 8), 169, (4, 2), True, (2, 2), ("rem", "mult"), False, "the same with an odd H: a stage step of more than a sample (qU = 1) together with a non-zero wrap correction (dWrap = one image row)"),
    _c("stage", (3, 20, 8), 35, (4, 2), True, (2, 2), ("lt", "rem"), True, "pair (4, 2), H > W: UPS = 10 and 5 for the CPRs of an 8 x 8 window; U = 8 over UPS = 5"),
    _c("stage", (3, 10, 10), 85, (5, 2), True, (2, 2), ("lt", "mult"), False, "pair (5, 2) on one network, ragged last stage (425 rows, U = 4)"),
    _c("stage", (3, 12, 12), 43, (6, 3), True, (3, 2), ("lt", "mult"), True, "pair (6, 3); CPR 3 as the second map with two stages"),
    _c("stage", (3, 14, 14), 43, (7, 3), True, (3, 2), ("lt", "mult"), True, "pair (7, 3), ragged (301 rows, U = 2)", ("alternate", "all-but-one"), True),
    _c("stage", (3, 16, 16), 22, (8, 4), True, (2, 2), ("lt", "eq"), True, "pair (8, 4); CPR 4 as the second map with two stages, U = UPS"),
    _c("stage", (3, 18, 18), 22, (9, 4), True, (2, 2), ("lt", "eq"), True, "pair (9, 4)", ("alternate", "all-but-one")),
    _c("stage", (3, 20, 20), 18, (10, 5), True, (2, 2), ("lt", "lt"), True, "pair (10, 5), both maps wrap inside a sample"),
    _c("stage", (3, 4, 20), 86, (10, 5), True, (2, 2), ("eq", "mult"), False, "pair (10, 5), H < W: UPS = 2 and 1 for the CPRs of a 20 x 20 window"),
    _c("stage", (3, 19, 22), 19, (11, 5), False, (2, 1), ("lt", "eq"), True, "CPR 11 (the widest the row-split kernels take), two launches: (11, 5) is no pair"),
    # the general kernel under the default switches: windows of more than 23 columns
    _c("general", (3, 4, 24), 9, (0, 6), False, (0, 1), ("-", "mult"), False, "W / 2 = 12: wgrad3_kernel for the window, CPR 6 alone for its 2 x 12 map"),
    _c("general", (3, 5, 48), 5, (0, 0), False, (0, 0), ("-", "-"), True, "W / 2 = 24, W / 4 = 12: wgrad3_kernel for both maps"),
    # CMLPL_WGRAD3_RG = 1, 2: one or two workgroups walk the whole batch
    _c("few", (3, 7, 7), 9, (3, 1), False, (1, 1), ("mult", "mult"), False, "odd window"),
    _c("few", (4, 10, 6), 7, (3, 1), False, (1, 1), ("rem", "mult"), False, "H != W; two workgroups split in mid-sample (35 rows, 18 + 17)"),
    _c("few", (3, 11, 9), 6, (4, 2), True, (1, 1), ("lt", "mult"), False, "pair (4, 2), odd, H != W; two workgroups split in mid-sample (30 rows, 16 + 14)"),
    # the compacted body where both 512-wide loops of wgrad3b_run take a second trip (more than 512 rows): the smallest
    # window whose step leaves the maxima table with few channels is 9 x 15 (the eight-tile per-sample kernels)
    _c("skip", (3, 9, 15), 600, (7, 3), True, (19, 10), ("lt", "mult"), True, "600 rows: second trip of the maxima fold and of the list build", ("third",)),
]


def under_switches(case):
    """(cpr, b3, pair, lower limits of the stages or None) of the case under the CMLPL_WGRAD3_* switches of this process"""
    env = lambda k, d: int(os.environ.get(k, d) or d)
    cpr, b3, pair, stages = case.cpr, tuple(1 if c else 0 for c in case.cpr), case.pair, case.stages
    if env("CMLPL_WGRAD3_R", "1") == 0:
        return (0, 0), (0, 0), False, None
    if env("CMLPL_WGRAD3_B3", "1") == 0:                 # wgrad3r_kernel exists for CPR 2 and 5 only
        cpr = tuple(c if c in (2, 5) else 0 for c in cpr)
        # (alone on 85 workgroups per kernel row, U = 8 / 4 pooled rows per stage: a "stage" case whose window has CPR 2 or
        #  5 still walks two stages or more of it)
        return cpr, (0, 0), False, (2 if case.tag == "stage" and cpr[0] else 0, 0)
    if env("CMLPL_WGRAD3_PAIR", "1") == 0 and pair:      # alone, a map has 85 workgroups per kernel row, not 64 or 21
        pair, stages = False, (2 if case.tag == "stage" else 1, 1)
    if env("CMLPL_WGRAD3_RG", "0") > 0 and cpr[0]:       # a handful of workgroups: the window's map in several stages each
        stages = (max(stages[0], 2), stages[1])
    return cpr, b3, pair, stages


def check_plan(case, plan):
    """the plan must be the case's regime (asserted before any number is compared)"""
    cpr, b3, pair, stages = under_switches(case)
    H = case.shape[1]
    assert tuple(m.cpr for m in plan.maps) == cpr and tuple(m.b3 for m in plan.maps) == b3 and plan.pair == pair, plan
    for m, ups, geo, c in zip(plan.maps, (H // 2, H // 4), case.geo, cpr):
        if c and m.b3:
            assert m.U == wg3b_U(c) and geometry(m.U, ups) == geo, (m, ups, geo)
        if c:
            assert m.UPG % m.U == 0, m
    if stages is not None:
        assert all(m.stages >= s for m, s in zip(plan.maps, stages)), (plan, stages)
