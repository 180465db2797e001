"""CPU: the planner of csrc/ntxent.hip (plan_ntxent, asked through cmlpl_debug_ntxent_plan) held to a table written by
hand, the case table of tests/ntxent_cases.py that tests/test_gpu_ntxent_envelope.py runs on the GPU, the reference's tie
to oracle.ntxent_loss and the conditions of every input.  Host arithmetic and CPU tensors: the library is loaded without
a device.

WHERE THE LIMITS LIE, from the LDS formulas of the two gradient kernels (floats; N2 = 2B, N2p = N2 rounded up to 64):

  vector   iden[N2] + W[8][N2] + red[64] + inrm[N2] = 10 N2 + 64 floats in 64 KiB = 16384 floats:
           10 N2 <= 16320, N2 <= 1632: B = 816 runs (65536 bytes exactly), B = 817 is refused.
  MFMA     ceil4(2 N2 + 128) + 16 N2p + 2 KC (64 NCW + 16) floats in 160 KiB = 40960 floats.
           NCW = 1, KC = 64: the chunks take 2 * 64 * 80 = 10240, so ceil4(2 N2 + 128) + 16 N2p <= 30720.
             N2p = 1664: 26624 + 2 * 1664 + 128 = 30080 fits; N2p = 1728: 27648 + 2 * 1666 + 128 = 31108 does not:
             B = 832 runs, B = 833 does not fit -- and is past the vector kernel too: refused.  B = 817 .. 832 run on
             the MFMA kernel alone (aligned rows only).
           NCW = 2, KC = 64: chunks 2 * 64 * 144 = 18432, rest <= 22528.  N2p = 1216: 19456 + 2560 = 22016 fits;
             N2p = 1280: 20480 + 2 * 1218 + 128 = 23044 does not: a forced NCW = 2 holds B <= 608, B = 609 goes to the
             vector kernel.
           NCW = 4, KC = 32: chunks 2 * 32 * 272 = 17408, rest <= 23552.  N2p = 1280: 20480 + 2688 = 23168 fits;
             N2p = 1344: 21504 + 2 * 1282 + 128 = 24196 does not: a forced NCW = 4 holds B <= 640, B = 641 goes to the
             vector kernel.
  planner  the widest slice with ceil(N2 / 16) ceil(D / (64 NCW)) >= 256 workgroups that fits.  With 32 row groups
           (B = 249: N2 = 498) NCW = 2 needs ceil(D / 128) >= 8: D = 900 is the first multiple of 4 (896: 7 slices, 224
           workgroups); B = 248 has 31 row groups, 248 workgroups.  With 64 row groups (B = 505: N2 = 1010) NCW = 4 needs
           ceil(D / 256) >= 4: D = 772 (768: 3 slices, 192); B = 504 has 63 row groups, 252 workgroups.
           B = 609, D = 1024: 128-column slices no longer fit, 256-column slices (77 x 4 workgroups) do -- NCW = 4;
           B = 641, D = 1024: neither fits, the planner stays at 64 columns."""
import os

import pytest
import torch

from cmlpl_amd import _lib
from oracle import cmlpl_oracle as O
from tests import ntxent_cases as N

MFMA0, NCW = ("CMLPL_NTX_MFMA", "0"), lambda v: ("CMLPL_NTX_NCW", str(v))
E = N.E_ARG
# (B, D, aligned, switches) -> route, NCW, KC, waves, sim grid x y, gradient grid x y, gradient LDS bytes, CT
TABLE = [
    # ---- which kernel
    (9, 36, 1, (), (1, 1, 64, 4, 1, 2, 2, 1, 45712, 1)),
    (9, 37, 0, (), (0, 0, 0, 4, 1, 2, 3, 1, 976, 1)),                         # D % 4 != 0
    (9, 37, 1, (), (0, 0, 0, 4, 1, 2, 3, 1, 976, 1)),                         # ... whatever `aligned` claims
    (9, 36, 0, (), (0, 0, 0, 4, 1, 2, 3, 1, 976, 1)),                         # D % 4 == 0, a pointer off a 16-byte boundary
    (9, 36, 1, (MFMA0,), (0, 0, 0, 4, 1, 2, 3, 1, 976, 1)),
    # ---- the planner's thresholds
    (248, 900, 1, (), (1, 1, 64, 4, 16, 31, 31, 15, 78208, 16)),
    (249, 896, 1, (), (1, 1, 64, 4, 16, 32, 32, 14, 78224, 16)),
    (249, 900, 1, (), (1, 2, 64, 4, 16, 32, 32, 8, 110992, 16)),              # the first 128-column slices
    (504, 772, 1, (), (1, 2, 64, 4, 32, 63, 63, 7, 147840, 32)),
    (505, 768, 1, (), (1, 2, 64, 4, 32, 64, 64, 6, 147856, 32)),
    (505, 772, 1, (), (1, 4, 32, 8, 32, 64, 64, 4, 143760, 32)),              # the first 256-column slices
    (609, 1024, 1, (), (1, 4, 32, 8, 39, 77, 77, 4, 161808, 39)),             # 128 columns do not fit, 256 do
    (641, 1024, 1, (), (1, 1, 64, 4, 41, 81, 81, 16, 137744, 41)),            # neither fits
    (249, 900, 1, (MFMA0,), (0, 0, 0, 4, 16, 32, 63, 4, 20176, 16)),
    # ---- a forced slice that fits, and one that does not
    (33, 260, 1, (NCW(4),), (1, 4, 32, 8, 3, 5, 5, 2, 78864, 3)),
    (33, 260, 1, (NCW(2),), (1, 2, 64, 4, 3, 5, 5, 3, 82960, 3)),
    (33, 260, 1, (NCW(1),), (1, 1, 64, 4, 3, 5, 5, 5, 50192, 3)),
    (33, 260, 1, (NCW(3),), (1, 1, 64, 4, 3, 5, 5, 5, 50192, 3)),             # any other value: 64 columns
    (505, 772, 1, (NCW(1),), (1, 1, 64, 4, 32, 64, 64, 13, 115088, 32)),
    (608, 8, 1, (NCW(2),), (1, 2, 64, 4, 38, 76, 76, 1, 161792, 38)),
    (609, 8, 1, (NCW(2),), (0, 0, 0, 4, 39, 77, 153, 1, 48976, 39)),
    (640, 8, 1, (NCW(4),), (1, 4, 32, 8, 40, 80, 80, 1, 162304, 40)),
    (641, 8, 1, (NCW(4),), (0, 0, 0, 4, 41, 81, 161, 1, 51536, 41)),
    # ---- the last B that runs and the first that is refused, on each route
    (816, 5, 0, (), (0, 0, 0, 4, 51, 102, 204, 1, 65536, 51)),
    (817, 5, 0, (), E),
    (816, 8, 0, (), (0, 0, 0, 4, 51, 102, 204, 1, 65536, 51)),
    (817, 8, 0, (), E),
    (816, 8, 1, (MFMA0,), (0, 0, 0, 4, 51, 102, 204, 1, 65536, 51)),
    (817, 8, 1, (MFMA0,), E),
    (817, 8, 1, (), (1, 1, 64, 4, 52, 103, 103, 1, 161040, 52)),
    (832, 8, 1, (), (1, 1, 64, 4, 52, 104, 104, 1, 161280, 52)),
    (833, 8, 1, (), E),
    (833, 8, 1, (NCW(2),), E),
    (833, 1024, 1, (), E),
    (100000, 8, 1, (), E),
    # ---- not a batch
    (0, 8, 1, (), E), (8, 0, 1, (), E), (-1, -1, 0, (), E),
]


@pytest.fixture
def switches():
    """set CMLPL_* switches for one test; the environment and the library's table are as before when it ends"""
    lib = _lib.load()
    saved = {k: os.environ.get(k) for k in N.SWITCHES}

    def put(env):
        for k in N.SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(dict(env))
        lib.cmlpl_debug_reload_switches()
    put({})
    yield put
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    lib.cmlpl_debug_reload_switches()


@pytest.mark.parametrize("B,D,aligned,env,want", TABLE,
                         ids=[f"{B}-{D}-{a}-" + "-".join(v for _, v in env) for B, D, a, env, _ in TABLE])
def test_plan_is_the_hand_written_one(B, D, aligned, env, want, switches):
    switches(env)
    assert N.ntxent_plan(B, D, aligned) == want


def test_the_restated_formulas_give_the_hand_written_plans():
    """full_plan / mfma_lds / vector_lds (what the GPU table is checked with) against the same hand-written rows"""
    for B, D, aligned, env, want in TABLE:
        if want != E:
            assert N.full_plan(B, D, want[0], want[1]) == want, (B, D, env)
    assert N.vector_lds(2 * N.LAST_VECTOR) == N.LDS_VECTOR < N.vector_lds(2 * N.LAST_VECTOR + 2)
    assert N.mfma_lds(2 * N.LAST_MFMA, 1) <= N.LDS_MAX < N.mfma_lds(2 * N.LAST_MFMA + 2, 1)
    assert N.mfma_lds(2 * 608, 2) <= N.LDS_MAX < N.mfma_lds(2 * 609, 2)
    assert N.mfma_lds(2 * 640, 4) <= N.LDS_MAX < N.mfma_lds(2 * 641, 4)


@pytest.mark.parametrize("case", N.CASES, ids=[c.name for c in N.CASES])
def test_plan_names_the_route_of_the_case(case, switches):
    switches(case.env)
    assert N.ntxent_plan(case.B, case.D, case.aligned) == N.full_plan(case.B, case.D, case.route, case.ncw)


def test_refused_shapes_and_the_routes_of_the_agreement_runs(switches):
    for B, D, _ in N.REFUSED:
        assert N.ntxent_plan(B, D, D % 4 == 0) == E and N.ntxent_plan(B - 1, D, D % 4 == 0) != E
        assert _lib.load().cmlpl_ntxent_workspace_bytes(B, D) > 0          # (the workspace question is answered all the same)
    for B, D in N.ALL_ROUTES:
        got = set()
        for env in N.ROUTE_ENVS:
            switches(env)
            got.add(N.ntxent_plan(B, D, True)[:2])
        assert got == {(0, 0), (1, 1), (1, 2), (1, 4)}, (B, D, got)


def test_the_table_reaches_every_edge_it_names():
    by = lambda pred: [c for c in N.CASES if pred(c)]
    plain = by(lambda c: c.family == "a" and c.T == 0.5 and not c.env and c.offs == (0, 0))
    for D in (36, 37):
        assert {c.B for c in plain if c.D == D} >= {1, 2, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33}
    assert {c.D for c in plain if c.B == 9} >= {1, 2, 3, 4, 5, 31, 32, 33, 60, 64, 68, 96, 100, 127, 128, 129, 132, 255,
                                                 256, 257, 260}
    for ncw in (1, 2, 4):
        forced = by(lambda c: c.env == (NCW(ncw),) and c.route == N.MFMA and c.ncw == ncw)
        for D in (260, 64):
            assert {c.B for c in forced if c.D == D} >= {32, 33, 64, 65, 96, 97, 128, 129, 160}
    for D, route in ((8, N.MFMA), (6, N.VECTOR)):
        assert {c.B for c in plain if c.D == D and c.route == route} >= {129, 257, 513}
    assert any(c.B == 257 and c.ncw == 4 for c in N.CASES)
    assert {(c.B, c.D, c.ncw) for c in plain} >= {(*N.NCW2_FIRST, 2), (*N.NCW4_FIRST, 4), (N.LAST_MFMA, 8, 1), (N.LAST_VECTOR, 5, 0)}
    assert {c.offs for c in N.CASES if c.D == 64 and c.route == N.VECTOR} >= {(1, 1), (1, 0), (0, 1)}
    for D, route in ((68, N.MFMA), (67, N.VECTOR)):
        fam = {(c.family, c.T) for c in N.CASES if (c.B, c.D, c.route) == (24, D, route)}
        assert fam >= {("b", 0.5), ("c", 0.5), ("d", 0.5), ("e", 0.5), ("f", 0.5), ("g", 0.2), ("a", 0.05), ("d", 0.05), ("f", 0.05)}
    assert min(c.T for c in N.CASES) == 0.05


def test_inputs_are_what_the_families_promise():
    ei, ej = N.inputs("b", 24, 68)
    n = ei.double().norm(dim=1)
    assert float(n.min()) < 2e-5 and float(n.max()) > 3e3 and float(ej.double().norm(dim=1)[0]) > 3e3
    ei, ej = N.inputs("c", 24, 68)
    assert int((ei.abs().sum(1) == 0).sum()) == 1 and bool((ej.abs().sum(1) > 0).all())
    ei, ej = N.inputs("d", 24, 68)
    assert torch.equal(ei[18], ei[3]) and len({tuple(r.tolist()) for r in ei}) == 23
    ei, ej = N.inputs("e", 24, 68)
    assert torch.equal(ei, ej)
    ei, ej = N.inputs("f", 24, 68)
    assert torch.equal(ei, -ej)
    ei, ej = N.inputs("g", 24, 68)
    assert 0 < float((ej - ei).abs().max()) < 0.6


def test_reference_is_the_oracle_in_matmul_form():
    """fp64, (B, D, T) = (9, 37, 0.4): loss and both gradients within 1e-12 of oracle.ntxent_loss"""
    ei, ej = N.inputs("a", 9, 37)
    ref, _ = N.reference(ei, ej, 0.4, torch.float64)
    xi, xj = ei.double().requires_grad_(True), ej.double().requires_grad_(True)
    loss = O.ntxent_loss(xi, xj, 0.4)
    loss.backward()
    d = dict(loss=float((ref["loss"] - loss.detach()).abs()), grad_i=float((ref["grad_i"] - xi.grad).abs().max()),
             grad_j=float((ref["grad_j"] - xj.grad).abs().max()))
    print(d)
    assert max(d.values()) <= 1e-12, d


@pytest.mark.parametrize("key", sorted({c.key for c in N.CASES}), ids=lambda k: "-".join(str(v) for v in k))
def test_inputs_meet_their_conditions(key):
    """fp32 and fp64 reference within BOUND / 8, finite fp32 denominators, an unsaturated loss (asserted in `prepared`);
    a gradient the reference has exactly zero (B = 1) is still given a scale"""
    _, ref, scale, d32 = N.prepared(key)
    print(key, {k: f"{v:.2e}" for k, v in d32.items()}, f"loss {float(ref['loss']):.4g}")
    if key[1] == 1:
        assert float(ref["grad_i"].abs().max()) <= 1e-14 * float(scale.max())
