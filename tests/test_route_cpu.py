"""CPU: the router (route_net in conv3x3.hip, asked through cmlpl_debug_route) against the shape-envelope table.

Until the router existed the table's regimes could be checked on a GPU only, by counting launches
(tests/test_gpu_shape_envelope.py).  The decision is host arithmetic: for every case the route must name the case's
forward and backward regime, its eight-tile flag and its four general plans under the default switches, and what
`_under_switches` / `_forced_s` expect under each forced setting tests/test_gpu_env_paths.py runs the cases with.  The
library plans for 256 compute units where it finds no device."""
import ctypes as C
import os

import pytest

from cmlpl_amd import _lib
from tests.envelope_cases import CASES, _forced_s, _under_switches

ROUTE_INTS = 30
SWITCHES = ("CMLPL_CONV3_S", "CMLPL_FUSE_TAIL", "CMLPL_FUSE_CONV0_BWD")


class Route:
    def __init__(self, case):
        out = (C.c_int * ROUTE_INTS)()
        cs = _lib.Shape(*case.shape)
        _lib.check("cmlpl_debug_route", _lib.load().cmlpl_debug_route(C.byref(cs), 1, case.n, out))
        o = list(out)
        self.fwd, self.bwd, self.big = "ABC"[o[0]], "ABC"[o[1]], bool(o[2])
        self.fwd_ps, self.bwd_ps = tuple(o[3:6]), tuple(o[6:9])                 # (waves, tiles per wave, two-piece)
        self.plans = tuple(tuple(o[9 + 5 * i: 12 + 5 * i]) for i in range(4))   # (S, tiles per wave, waves)
        self.ks = tuple(o[12 + 5 * i] for i in range(4))
        self.h2x = tuple(o[13 + 5 * i] for i in range(4))
        self.stats = o[29]


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


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_route_names_the_regime_of_the_case(case, switches):
    r = Route(case)
    assert (r.fwd, r.bwd, r.big, r.plans) == (case.fwd, case.bwd, case.big, case.plans)
    # the per-sample launches exist in regimes A and B only, and eight tiles only with their tail / head
    assert (r.fwd_ps == (0, 0, 0)) == (r.fwd == "C") and (r.bwd_ps == (0, 0, 0)) == (r.bwd == "C")
    assert r.big == ((r.fwd == "A" and r.fwd_ps[:2] == (8, 2)) or (r.bwd == "A" and r.bwd_ps[:2] == (8, 2)))
    # the statistics table is written only where every launch that sees one of its images is a two-piece kernel
    if r.stats:
        assert (r.fwd, r.bwd) == ("A", "A") and r.fwd_ps[2] and r.bwd_ps[2] or (r.fwd, r.bwd) == ("C", "C") and all(r.h2x)


@pytest.mark.parametrize("s", (2, 3, 5, 16))
@pytest.mark.parametrize("case", [c for c in CASES if c.tag == "forceS"], ids=lambda c: c.id)
def test_route_under_a_forced_sample_count(case, s, switches):
    switches({"CMLPL_CONV3_S": str(s)})
    fwd, bwd, force_s = _under_switches(case)
    r = Route(case)
    assert force_s == s and (r.fwd, r.bwd) == (fwd, bwd) == ("C", "C")
    assert tuple(p[0] for p in r.plans) == _forced_s(case, s), r.plans


@pytest.mark.parametrize("env", ({"CMLPL_FUSE_TAIL": "0"}, {"CMLPL_FUSE_CONV0_BWD": "0"}), ids=lambda e: "-".join(e))
@pytest.mark.parametrize("case", [c for c in CASES if c.fwd == "A"], ids=lambda c: c.id)
def test_route_of_the_whole_sample_cases_under_the_fusion_switches(case, env, switches):
    switches(env)
    fwd, bwd, force_s = _under_switches(case)
    r = Route(case)
    assert force_s == 0 and (r.fwd, r.bwd) == (fwd, bwd)
    assert r.plans == case.plans                      # (the general plans do not depend on these switches)
    assert r.big == (case.big and "A" in (fwd, bwd))
