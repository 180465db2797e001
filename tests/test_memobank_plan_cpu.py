"""CPU: the two planners of csrc/memobank.hip (plan_unsup / plan_mb_onepass, asked through cmlpl_debug_unsup_plan and
cmlpl_debug_memobank_plan) held to the regime tables of tests/memobank_cases.py that tests/test_gpu_memobank_envelope.py
runs on the GPU, their boundaries and refusals, and the tables themselves: every input condition the cases promise is
there, every route sees every data variant, every kernel of the file is named by a run.  Host arithmetic and CPU
tensors: the library is loaded without a device."""
import os

import pytest
import torch

from cmlpl_amd import _lib
from tests import memobank_cases as M


@pytest.fixture
def switches():
    """set CMLPL_* switches for one test; the environment and the library's table are as before when it ends"""
    lib = _lib.load()
    saved = {k: os.environ.get(k) for k in M.SWITCHES}

    def put(env):
        for k in M.SWITCHES:
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


@pytest.mark.parametrize("run", M.URUNS, ids=[r.id for r in M.URUNS])
def test_unsup_plan_names_the_route_of_the_run(run, switches):
    switches(run.env)
    assert M.unsup_plan(run.case.B, run.case.K) == (run.route, run.regrows)


def test_unsup_plan_boundaries_and_refusals(switches):
    for env in ({}, {"CMLPL_UNSUP_3L": "0"}, {"CMLPL_UNSUP_ONEWG": "0"}, {"CMLPL_UNSUP_ONEWG": "0", "CMLPL_UNSUP_3L": "0"}):
        switches(env)
        for K in (1, 16, 17, 64):
            rr = 1 if K <= 16 else 0
            for B in (1, 2, 1023, 1024, 1025, 4096, 8192, 8193, 100000):
                if "CMLPL_UNSUP_ONEWG" in env or B > 8192:
                    want = (M.FIVE, 0)
                elif B <= 1024 or "CMLPL_UNSUP_3L" in env:
                    want = (M.ONEWG, rr)
                else:
                    want = (M.THREE, rr)
                assert M.unsup_plan(B, K) == want, (env, B, K)
        assert M.unsup_plan(0, 9) == M.E_ARG and M.unsup_plan(5, 0) == M.E_ARG and M.unsup_plan(-1, -1) == M.E_ARG


def test_every_route_sees_every_data_variant():
    for route in (M.ONEWG, M.THREE, M.FIVE):
        cases = [r.case for r in M.URUNS if r.route == route]
        assert {"tie_in", "tie_lo", "tie_above", "n1", "n2", ""} <= {c.variant for c in cases}, route
        assert {"zero", "low", "high"} <= {c.g for c in cases}, route
        assert any(c.percent == 100.0 for c in cases) and any(c.ignored and not c.variant for c in cases), route
        assert any(c.name.endswith("g0") for c in cases), route
        assert {0, 1} == {r.regrows for r in M.URUNS if r.route == route} or route == M.FIVE
    table = {(r.route, r.regrows, r.case.B, r.case.K) for r in M.URUNS if not r.env}
    for B, K in ((1, 9), (63, 2), (65, 16), (1024, 9)):
        assert (M.ONEWG, 1, B, K) in table
    assert (M.ONEWG, 0, 1024, 17) in table
    assert {(M.THREE, 1, 1025, 9), (M.THREE, 1, 8192, 16), (M.THREE, 0, 1025, 17), (M.THREE, 0, 8192, 17)} <= table
    assert {(M.FIVE, 0, 8193, 9), (M.FIVE, 0, 8193, 17)} <= table
    forced = {(r.route, r.case.B, r.case.K) for r in M.URUNS if r.env}
    assert {(M.FIVE, 1, 9), (M.FIVE, 255, 9), (M.FIVE, 257, 9)} <= forced
    assert {(M.ONEWG, 1025, 9), (M.ONEWG, 1025, 17), (M.ONEWG, 8192, 9), (M.ONEWG, 8192, 17)} <= forced


@pytest.mark.parametrize("case", M.UCASES, ids=[c.name for c in M.UCASES])
def test_unsup_inputs_meet_their_conditions(case):
    _, target, teacher = M.unsup_inputs(case)
    M.unsup_conditions(case, target, teacher)


@pytest.mark.parametrize("run", M.CRUNS, ids=[r.id for r in M.CRUNS])
def test_memobank_plan_names_the_kernel_of_the_run(run, switches):
    switches(run.env)
    c = run.case
    assert M.memobank_plan(c.D, c.K, c.Q, c.NN) == (run.kernel, *M.memobank_lds(c, run.kernel))


def test_memobank_plan_over_the_whole_range(switches):
    """the fast kernel exactly where the header says: D a multiple of 4 and <= 1024, K <= 64,
    ceil((negatives + 1) / 4) * ceil(D / 256) <= 16; every instantiation is reachable"""
    seen = set()
    for D in list(range(1, 40)) + list(range(250, 270)) + list(range(508, 520)) + list(range(764, 776)) + list(range(1020, 1032)):
        for NN in (1, 2, 3, 14, 15, 16, 18, 19, 20, 30, 31, 32, 50, 62, 63, 64, 126, 127):
            for K in (1, 6, 64, 65):
                nch = -(-D // 256)
                fast = D % 4 == 0 and D <= 1024 and K <= 64 and -(-(NN + 1) // 4) * nch <= 16
                want = nch if fast else M.GENERAL
                plan = M.memobank_plan(D, K, 16, NN)
                assert plan == (want, 16 * D if fast else 4 * D, 4 * K * 16), (D, NN, K, plan)
                seen.add(plan[0])
    assert seen == {0, 1, 2, 3, 4}
    switches({"CMLPL_MB_FAST": "0"})
    assert M.memobank_plan(256, 6, 256, 50)[0] == M.GENERAL


def test_memobank_plan_refuses_what_the_launcher_refuses(switches):
    """... and a refusal is made before anything is launched (tests/test_gpu_memobank_envelope.py holds the call to it):
    K * queries beyond the scatter's 64 KiB of slots, more than 127 negatives, more than 1024 classes"""
    assert M.memobank_plan(8, 64, 256, 15) == (1, 128, 65536)          # exactly the limit: runs
    for D, K, Q, NN in ((8, 65, 256, 15), (8, 64, 257, 15), (8, 1024, 17, 15), (8, 1, 16385, 15), (8, 6, 64, 128),
                        (8, 6, 64, 0), (8, 1025, 1, 15), (0, 6, 64, 15), (8, 0, 64, 15), (8, 6, 0, 15), (50000, 6, 64, 15)):
        assert M.memobank_plan(D, K, Q, NN) == M.E_ARG, (D, K, Q, NN)


def test_contra_inputs_show_every_condition():
    seen = set()
    for case in M.CCASES:
        inp = M.contra_inputs(case)
        res, _ = M.run_oracle(case, inp, torch.float64)
        feats = M.contra_features(case, inp, res)
        if case.absent and case.Q == 256:
            assert feats == set(M.FEATURES), (case.name, set(M.FEATURES) - feats)
        assert len(inp["plan"]) >= 3 and float(res["loss"].detach()) > 0, case.name
        seen |= feats
    assert seen == set(M.FEATURES)
    assert {c.mom for c in M.CCASES} == {"", "on", "zero"} and {c.N for c in M.CCASES} == {300, 301}
    assert any(c.Q == 1 for c in M.CCASES) and all(not M.CASE_BY_NAME[n].mom for n in M.STAGED)
    assert {M.CASE_BY_NAME[n].kernel for n in M.IN_KERNEL} == {1, 2, 3, 4}
    staged = [M.CASE_BY_NAME[n] for n in M.STAGED]
    assert any(c.NN == 127 for c in staged) and any(c.Q == 100 and c.absent for c in staged)


def test_every_kernel_of_the_file_is_named_by_a_run():
    whys = " ".join([r.why for r in M.URUNS] + [r.why for r in M.CRUNS] + [M.STAGED_WHY, M.PUSH_WHY])
    assert [k for k in M.KERNELS if k not in whys] == []
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "memobank.hip")).read()
    import re
    names = set(re.findall(r"\bvoid ((?:mb|us)_\w+_kernel)\(", src))
    assert names == {k.split("<")[0] for k in M.KERNELS}, names ^ {k.split("<")[0] for k in M.KERNELS}
