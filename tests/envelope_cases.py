"""The shape-envelope table: one case per planner regime of the network kernels, and what the CMLPL_* switches make of
each.  Plain data and arithmetic (no device, no library): tests/test_gpu_shape_envelope.py runs the cases on the GPU
against the fp64 oracle, tests/test_route_cpu.py holds the router's answers to the same table without one."""
import os
from typing import NamedTuple


class Case(NamedTuple):
    tag: str            # "table": the envelope; "forceS": also run under CMLPL_CONV3_S (test_gpu_env_paths.py)
    shape: tuple        # (C, H, W, bands, K)
    n: int
    fwd: str            # regime under the default switches
    bwd: str
    big: bool           # the eight-tile per-sample kernels (129 .. 256 window pixels)
    plans: tuple        # plan_conv3's (samples per workgroup, tiles per wave (0: split tile), waves) for conv1 forward,
                        # conv1 data gradient, conv2 forward, conv2 data gradient -- under the default switches
    why: str

    @property
    def id(self):
        return f"{self.tag}-fwd{self.fwd}_bwd{self.bwd}-" + "x".join(map(str, self.shape)) + f"-n{self.n}"


SPLIT, KS = (1, 0, 4), (1, 1, 4)      # one sample: the one-tile split kernel / one tile per wave
CASES = [
    Case("table", (3, 4, 4, 5, 2), 7, "C", "C", False, (SPLIT,) * 4, "split tile for conv1, conv2 on a 2 x 2 map, P4 = 1"),
    Case("table", (5, 5, 5, 4, 3), 9, "C", "C", False, (SPLIT,) * 4, "odd window, pooled 2 x 2"),
    Case("table", (7, 6, 6, 6, 3), 11, "B", "C", False, (KS, KS, SPLIT, SPLIT), "fused conv0 + conv1, conv2 on 3 x 3; C < 32: general backward"),
    Case("table", (40, 6, 6, 6, 3), 11, "B", "B", False, (KS, KS, SPLIT, SPLIT), "B forward with the B backward (C >= 32)"),
    Case("table", (4, 7, 7, 3, 4), 6, "B", "C", False, (KS, KS, SPLIT, SPLIT), "B, odd window"),
    Case("table", (36, 7, 7, 3, 4), 6, "B", "B", False, (KS, KS, SPLIT, SPLIT), "B / B, odd window"),
    Case("table", (9, 8, 16, 9, 5), 10, "B", "C", False, (KS, KS, SPLIT, SPLIT), "B at exactly 128 pixels, W = 16 divide"),
    Case("table", (9, 16, 8, 9, 5), 10, "B", "C", False, (KS, KS, SPLIT, SPLIT), "B, transposed"),
    Case("table", (33, 9, 11, 7, 4), 13, "A", "B", False, (KS, KS, SPLIT, SPLIT), "A, H != W"),
    Case("table", (33, 11, 9, 7, 4), 13, "A", "B", False, (KS, KS, SPLIT, SPLIT), "A, transposed"),
    Case("table", (17, 10, 10, 17, 7), 21, "A", "C", False, (KS, KS, SPLIT, SPLIT), "A, even 10; C = 16 + 1"),
    Case("table", (6, 10, 13, 5, 3), 9, "A", "A", True, (KS, (1, 2, 4), SPLIT, SPLIT), "big, 130 pixels (the smallest)"),
    Case("table", (6, 12, 16, 5, 3), 9, "A", "A", True, ((1, 1, 8), (1, 1, 8), KS, KS), "big, P4 = 12 (the limit)"),
    Case("table", (6, 16, 12, 5, 3), 9, "A", "A", True, ((1, 1, 8), (1, 1, 8), KS, KS), "big, transposed"),
    Case("table", (5, 14, 14, 7, 4), 8, "A", "A", True, ((1, 1, 8), (1, 1, 8), KS, KS), "big, P2 = 49"),
    Case("table", (3, 17, 17, 5, 3), 5, "C", "C", False, ((1, 1, 8), (1, 2, 8), KS, KS), "general, odd; pooled 8 x 8"),
    Case("table", (3, 19, 19, 5, 3), 5, "C", "C", False, ((1, 2, 8), (1, 2, 8), KS, KS), "general, odd; pooled 9 x 9"),
    Case("table", (4, 20, 12, 6, 3), 5, "C", "C", False, ((1, 1, 8), (1, 1, 8), KS, KS), "H != W on the general kernels (P4 = 15: not big)"),
    Case("table", (1, 11, 11, 1, 1), 9, "A", "C", False, (KS, KS, SPLIT, SPLIT), "A with C = 1, bands = 1, K = 1"),
    Case("table", (256, 11, 11, 12, 64), 6, "A", "A", False, (KS, KS, SPLIT, SPLIT), "C and K at their limits"),
    Case("table", (128, 8, 8, 300, 9), 40, "A", "B", False, (KS, KS, SPLIT, SPLIT), "C = 128, bands > 256 (8 x 8 is fused: conv0a is not reached)"),
    Case("table", (128, 4, 4, 300, 9), 12, "C", "C", False, (SPLIT,) * 4, "conv0a's limit C = 128 on the general path, bands > 256"),
    Case("table", (129, 4, 4, 9, 3), 12, "C", "C", False, (SPLIT,) * 4, "just past conv0a's C on the general path: conv0_fwd_kernel"),
    Case("table", (129, 12, 12, 20, 9), 6, "A", "A", True, ((1, 2, 4), (1, 2, 4), KS, KS), "just past conv0a's C; big kernels with band passes"),
    Case("table", (3, 4, 4, 5, 2), 701, "C", "C", False, ((2, 0, 4), (2, 0, 4), (3, 0, 4), (3, 0, 4)),
         "the planner picks S > 1 by itself (more than 256 workgroups), ragged last workgroup"),
    # for the CMLPL_CONV3_S jobs: n % S != 0 at S = 2, 3, 5 and at what 16 comes to (14 | 16, 7 | 16, 5 | 14 images on the
    # windows | their pooled maps); fewer rows than a workgroup holds at 16
    Case("forceS", (5, 4, 4, 3, 4), 37, "C", "C", False, (SPLIT,) * 4, "multi-sample general kernels, ragged tail"),
    Case("forceS", (6, 6, 6, 4, 3), 11, "B", "C", False, (KS, KS, SPLIT, SPLIT), "multi-sample general kernels, ragged tail"),
    Case("forceS", (8, 8, 8, 12, 5), 7, "A", "C", False, (KS, KS, SPLIT, SPLIT), "multi-sample general kernels, ragged tail"),
    Case("forceS", (3, 4, 4, 5, 2), 13, "C", "C", False, (SPLIT,) * 4, "fewer rows than a forced workgroup holds"),
]


def _forced_s(case, s):
    """samples per workgroup of the four general launches under CMLPL_CONV3_S = s: s itself, or the most the map holds
    (plan_conv3: LDS of 160 KiB, at most four tiles per wave) -- a 4 x 4 window holds 14 images, its 2 x 2 map 16."""
    H, W = case.shape[1:3]

    def most(h, w, mode):
        px = (2 * (h // 2)) * (2 * (w // 2)) if mode == 0 else h * w
        best = 0
        for S in range(1, 17):
            mtw = ((S * px + 31) // 32 + 3) // 4
            if mtw > 4 or (S * (h + 2) * (w + 2) * 68 + 6144 + mtw * 128) * 4 > 160 * 1024:
                break
            best = S
        return min(s, best)
    return tuple(most(h, w, m) for h, w, m in ((H, W, 0), (H, W, 1), (H // 2, W // 2, 0), (H // 2, W // 2, 1)))


def _under_switches(case):
    """(forward regime, backward regime, forced samples per workgroup or 0) under the CMLPL_* switches of this process"""
    env = lambda k, d: int(os.environ.get(k, d) or d)
    fwd, bwd = case.fwd, case.bwd
    s = env("CMLPL_CONV3_S", "0")
    if s > 1 and not case.big:                      # the fused kernels need the one-sample plan
        return "C", "C", s
    if env("CMLPL_FUSE_TAIL", "1") == 0:
        if case.big:                                # the eight-tile kernels exist with their tail / head only
            fwd = bwd = "C"
        else:
            fwd = "B" if fwd == "A" else fwd
            bwd = "B" if bwd == "A" else bwd
    if env("CMLPL_FUSE_CONV0_BWD", "1") == 0:
        bwd = "C"
    return fwd, bwd, 0
