"""CPU: the planner of the 3x3 weight gradients (plan_wgrad3 / plan_wgrad3_both in wgrad3x3.hip, asked through
cmlpl_debug_wgrad3_plan) -- its invariants over every window the router accepts, and the regime table
(tests/wgrad_cases.py) that tests/test_gpu_wgrad_envelope.py runs on the GPU.  Host arithmetic: the library plans for
256 compute units where it finds no device.

What the sweep found about wide windows: the router accepts non-square windows of up to 82 columns (4 x 82), so W / 2
goes far beyond 11.  From W = 24 on the window's map takes the general wgrad3_kernel under the DEFAULT switches, and
from W = 48 on its pooled map does too; `test_wide_windows_take_the_general_kernel` records that, and the table has a
GPU case for either ("general")."""
import ctypes as C
import os

import pytest

from cmlpl_amd import _lib
from tests.wgrad_cases import CASES, LDS_MAX, MAXCPR, PAIRS, check_plan, read_plan, wg3b_U

SWITCHES = ("CMLPL_WGRAD3_RG", "CMLPL_WGRAD3_PG1", "CMLPL_WGRAD3_PG2", "CMLPL_WGRAD3_R", "CMLPL_WGRAD3_B3",
            "CMLPL_WGRAD3_PAIR", "CMLPL_WGRAD3_U", "CMLPL_WGRAD3_RU", "CMLPL_WGRAD3_CSPL", "CMLPL_F16X2", "CMLPL_ZERO_SKIP")
ROWS = (1, 2, 7, 64, 85, 86, 256, 513, 701, 1100)


def _accepted():
    lib = _lib.load()
    out = (C.c_int * 30)()
    return [(H, W) for H in range(4, 100) for W in range(4, 100)
            if lib.cmlpl_debug_route(C.byref(_lib.Shape(3, H, W, 4, 3)), 1, 7, out) == 0]


@pytest.fixture
def switches():
    """set CMLPL_* switches for one test; the environment and the library's table are as before when it ends"""
    lib = _lib.load()
    saved = {k: os.environ.get(k) for k in SWITCHES}

    def put(env):
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        lib.cmlpl_debug_reload_switches()
    put({})
    yield put
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    lib.cmlpl_debug_reload_switches()


def _invariants(H, W, nets, n, plan, forced_groups=None):
    """what must hold of a plan of the row-split kernels whatever the switches"""
    for m, h, w in zip(plan.maps, (H, H // 2), (W, W // 2)):
        where = (H, W, nets, n, m)
        assert m.lds <= LDS_MAX, where
        if w // 2 <= MAXCPR:
            assert m.cpr == w // 2 and m.b3 == 1, where
        else:
            assert m.cpr == 0 and m.b3 == 0 and m.cspl == 1, where      # the general kernel
            continue
        rows = n * (h // 2)
        assert m.G * m.UPG >= rows > (m.G - 1) * m.UPG, where          # no workgroup of the three-piece body is empty
        assert m.U == wg3b_U(m.cpr) and m.UPG % m.U == 0, where
        if forced_groups:
            assert m.G <= forced_groups, where
    cprs = tuple(m.cpr for m in plan.maps)
    assert plan.pair == (cprs in PAIRS), (H, W, cprs, plan.pair)
    if plan.pair:                                                      # "one round": both maps' workgroups at once
        assert (plan.maps[0].G + plan.maps[1].G) * 3 * nets <= plan.cus, (H, W, nets, n, plan)
    if plan.slist:
        assert plan.pair and H // 4 >= 2, (H, W, plan)


def test_planner_invariants_over_every_accepted_window(switches):
    acc = _accepted()
    assert len(acc) > 700 and (20, 20) in acc and (4, 4) in acc
    seen = set()
    for H, W in acc:
        for nets in (1, 2):
            for n in ROWS:
                plan = read_plan((3, H, W, 4, 3), nets, n)
                assert plan.cus >= 1
                _invariants(H, W, nets, n, plan)
                seen.update(m.cpr for m in plan.maps)
    assert seen == set(range(0, MAXCPR + 1))                # every instantiated CPR is reachable; 0 = the general kernel


@pytest.mark.parametrize("env", [{"CMLPL_WGRAD3_RG": "1"}, {"CMLPL_WGRAD3_RG": "2"}, {"CMLPL_WGRAD3_RG": "3"},
                                 {"CMLPL_WGRAD3_PG1": "16"}, {"CMLPL_WGRAD3_PG2": "8"},
                                 {"CMLPL_WGRAD3_PG1": "20", "CMLPL_WGRAD3_PG2": "12"}], ids=lambda e: "-".join(f"{k[13:]}{v}" for k, v in e.items()))
def test_planner_invariants_under_forced_group_counts(env, switches):
    """CMLPL_WGRAD3_RG: that many workgroups per network and kernel row for every map; _PG1 / _PG2: for the first / second
    map of a pair launch (values that leave the pair its one round on 256 units with two networks)"""
    switches(env)
    rg = int(env.get("CMLPL_WGRAD3_RG", "0"))
    for H, W in _accepted():
        for nets in (1, 2):
            for n in ROWS:
                plan = read_plan((3, H, W, 4, 3), nets, n)
                _invariants(H, W, nets, n, plan, forced_groups=rg)
                if plan.pair and "CMLPL_WGRAD3_PG1" in env:
                    assert plan.maps[0].G <= int(env["CMLPL_WGRAD3_PG1"])
                if plan.pair and "CMLPL_WGRAD3_PG2" in env:
                    assert plan.maps[1].G <= int(env["CMLPL_WGRAD3_PG2"])


def test_wide_windows_take_the_general_kernel(switches):
    """W / 2 > 11 exists among the accepted windows (H * W is what limits a window, not W): under the default switches the
    map then runs on wgrad3_kernel<1>, one unit of all the sample's rows where they fit"""
    acc = _accepted()
    wide = [(H, W) for H, W in acc if W // 2 > MAXCPR]
    assert wide and max(W for _, W in acc) == 82 and min(W for _, W in wide) == 24
    for H, W in wide:
        plan = read_plan((3, H, W, 4, 3), 1, 7)
        assert plan.maps[0].cpr == 0 and not plan.pair
        assert (plan.maps[1].cpr == 0) == (W // 4 > MAXCPR)


def test_which_kernels_run_alone_under_the_default_switches(switches):
    """wgrad3b_kernel<CPR> in a launch of its own: a window of 8 .. 21 columns takes the pair launch, so CPR 4 .. 10 run
    alone only as the POOLED map of a window too wide for the row-split kernels (24 .. 47 columns: CPR 6 .. 11) or of a
    22 / 23-column one (CPR 5, next to CPR 11).  CPR 4 alone is what no accepted window gives (CMLPL_WGRAD3_PAIR=0 does)."""
    first, second = set(), set()
    for H, W in _accepted():
        plan = read_plan((3, H, W, 4, 3), 1, 7)
        if not plan.pair:
            first.update(m.cpr for m in plan.maps[:1] if m.b3)
            second.update(m.cpr for m in plan.maps[1:] if m.b3)
    assert first == {2, 3, 11} and second == {1, 5, 6, 7, 8, 9, 10, 11}, (first, second)


@pytest.mark.parametrize("env", [{}, {"CMLPL_WGRAD3_PAIR": "0"}, {"CMLPL_WGRAD3_R": "0"}, {"CMLPL_WGRAD3_B3": "0"},
                                 {"CMLPL_WGRAD3_RG": "1"}, {"CMLPL_WGRAD3_RG": "2"}], ids=lambda e: "-".join(e) or "default")
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_plan_names_the_regime_of_the_case(case, env, switches):
    switches(env)
    plan = read_plan(case.shape, 1, case.n)
    check_plan(case, plan)
    if not env:
        assert tuple(m.stages for m in plan.maps) == case.stages      # (exactly, on 256 units)
        route = (C.c_int * 30)()
        _lib.check("cmlpl_debug_route", _lib.load().cmlpl_debug_route(C.byref(_lib.Shape(*case.shape)), 1, case.n, route))
        assert bool(route[29]) == case.two and plan.slist == (case.two and case.pair)


def test_every_kernel_of_the_table_runs_in_several_stages(switches):
    """the table itself: every CPR of wgrad3b_kernel the sweep can produce and every instantiated pair kernel in at least
    one case whose workgroups run two stages or more of that map (of both maps: the pairs)"""
    staged, pairs = set(), set()
    for case in CASES:
        plan = read_plan(case.shape, 1, case.n)
        staged.update(m.cpr for m in plan.maps if m.b3 and m.stages >= 2)
        if plan.pair and all(m.stages >= 2 for m in plan.maps):
            pairs.add(tuple(m.cpr for m in plan.maps))
    assert staged == set(range(1, MAXCPR + 1)), staged
    assert pairs == set(PAIRS), pairs
