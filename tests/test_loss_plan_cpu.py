"""CPU: the planner of the loss block's first launch (plan_loss_phase1 in loss.hip, the one function launch_loss_phase1
obeys, asked through cmlpl_debug_loss_plan) -- the regime table (tests/loss_cases.py) that
tests/test_gpu_loss_envelope.py runs on the GPU, the table's own coverage, and the planner's boundaries by sweep: 127 /
128 column tiles, 63 / 64 and 128 / 129 local rows, K = 32 / 33.  Host arithmetic: the library plans for 256 compute
units where it finds no device; nothing is launched."""
import os

import pytest

from cmlpl_amd import _lib
from tests.loss_cases import (BOTH_EPILOGUES, CASES, DEFAULT, KERNELS, PAIR16, PAIR32, RUNS, SWITCHES, TALL, WIDE, WIDE_SHAPES,
                              check_plan, read_plan)

ROWS = {PAIR16: 16, PAIR32: 32, TALL: 128}          # local rows per workgroup (the wide kernel: 32 MB)


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


def _covers(plan, nunl, maxc):
    """the grid covers every local row and every column, with no workgroup wholly outside either"""
    rows = 32 * plan.MB if plan.kernel == WIDE else ROWS[plan.kernel]
    cols = 32 * (4 // plan.MB) * plan.NBW if plan.kernel == WIDE else 32
    assert (plan.gy - 1) * rows < nunl <= plan.gy * rows, (plan, nunl)
    assert (plan.gx - 1) * cols < maxc <= plan.gx * cols, (plan, maxc)
    assert (plan.MB, plan.NBW) in WIDE_SHAPES if plan.kernel == WIDE else (plan.MB, plan.NBW) == (0, 0), plan


@pytest.mark.parametrize("run", RUNS, ids=[r.id for r in RUNS])
def test_plan_names_the_regime_of_the_run(run, switches):
    switches(run.env)
    c = run.case
    plan = read_plan(c.K, c.bt, c.btu, c.Q, c.smooth)
    print(run.id, run.why, plan)
    check_plan(run, plan)
    _covers(plan, c.btu, c.Q if c.smooth else c.btu)


def test_every_case_meets_the_tables_own_rules():
    assert len({c.name for c in CASES}) == len(CASES) and len({r.id for r in RUNS}) == len(RUNS)
    for c in CASES:
        assert c.Q >= c.bt + c.btu and 1 <= c.btu <= 2048 and 1 <= c.K <= 64, c
        assert c.adap == 0.9 if c.K == 1 else 0.5 <= c.adap <= 0.7, c
    assert [r.case for r in DEFAULT] == CASES and all(not r.env for r in DEFAULT)
    assert sum(1 for c in CASES if not c.smooth) == 1


def test_regimes_are_each_covered_twice():
    """every kernel in at least two runs, every kernel that has both epilogues with K <= 32 and with K > 32, every
    instantiation of the wide kernel, and either feature-gradient launch by shape and by switch"""
    for k, name in KERNELS.items():
        ks = [r.case.K for r in RUNS if r.kernel == k]
        assert len(ks) >= 2, name
        if k in BOTH_EPILOGUES:
            assert min(ks) <= 32 < max(ks), (name, ks)
        else:
            assert max(ks) <= 32, (name, ks)
    assert {(r.MB, r.NBW) for r in RUNS if r.kernel == WIDE} == set(WIDE_SHAPES)
    assert {(r.MB, r.NBW) for r in DEFAULT if r.kernel == WIDE} == {(2, 1), (4, 2)}          # the planner's own two
    assert any(r.kernel == TALL and not r.env and r.case.K > 32 for r in RUNS) and any(r.kernel == TALL and not r.env and r.case.K <= 32 for r in RUNS)
    assert {32, 33, 64, 1} <= {c.K for c in CASES}
    assert any(not r.case.lds_shape for r in RUNS) and any(r.case.lds_shape and not r.lds for r in RUNS) and any(r.lds for r in RUNS)


def test_the_wide_kernel_starts_at_128_column_tiles(switches):
    """Q = 4064 is 127 tiles, 4065 is 128: up to 128 local rows the planner goes from the 16-row kernel to the wide one
    there (K <= 32), to nothing else (K > 32, fewer than 64 rows); smoothing off, the banks' width does not count"""
    for Q in list(range(3900, 4300, 7)) + [4064, 4065]:
        tiles = (Q + 31) // 32
        for nunl in (1, 16, 63, 64, 100, 128):
            p = read_plan(9, 16, nunl, Q, True)
            assert p.ctiles == tiles and p.kernel == (WIDE if tiles >= 128 else PAIR16), (Q, nunl, p)
            _covers(p, nunl, Q)
            if tiles >= 128 and nunl <= 64:
                assert p.MB == 2, (Q, nunl, p)                                                      # 64 rows or fewer: never MB = 4
            off = read_plan(9, 16, nunl, Q, False)
            assert off.kernel == PAIR16 and off.ctiles == (nunl + 31) // 32 and off.gx == off.ctiles, (Q, nunl, off)
        p = read_plan(40, 16, 16, Q, True)
        assert p.kernel == PAIR32 and p.gx == tiles, (Q, p)
    assert read_plan(9, 16, 16, 4064, True).kernel == PAIR16 and read_plan(9, 16, 16, 4065, True).kernel == WIDE


def test_local_rows_63_64_and_128_129(switches):
    """from 128 column tiles on: the wide kernel up to 128 local rows and the tall one beyond (K <= 32); the tall kernel from
    64 local rows on where the wide kernels are refused (K > 32) -- local rows, not the global batch's"""
    Q = 4096
    for nunl in range(1, 300):
        for btu_g in (nunl, 4 * nunl):
            shard = (2 * btu_g, btu_g, 0, 2 * nunl, 0, nunl)
            if Q < 3 * btu_g:
                continue
            p = read_plan(9, 0, 0, Q, True, shard)
            assert p.kernel == (WIDE if nunl <= 128 else TALL), (nunl, btu_g, p)
            _covers(p, nunl, Q)
            q = read_plan(33, 0, 0, Q, True, shard)
            assert q.kernel == (PAIR32 if nunl < 64 else TALL) and (q.MB, q.NBW) == (0, 0), (nunl, btu_g, q)
            _covers(q, nunl, Q)
            assert p.lds_shape == q.lds_shape == (nunl % 4 == 0 and btu_g % 4 == 0), (nunl, btu_g, p)
    below = [read_plan(9, 16, n, 4032, True).kernel for n in (63, 64, 128, 129, 2048)]         # 126 tiles: rows decide nothing
    assert below == [PAIR16] * 5, below


def test_no_switch_puts_more_than_32_classes_on_a_kernel_without_the_shuffle_epilogue(switches):
    """pair_exp16_kernel and the wide kernels hold a [32 columns][K <= 32] probability tile: K = 33 .. 64 must stay on
    pair_exp_kernel or pair_exp_tall_kernel whatever is forced"""
    envs = [{}, {"CMLPL_PAIR_WIDE": "1"}, {"CMLPL_PAIR_WIDE": "1", "CMLPL_PAIR_MB": "4", "CMLPL_PAIR_NBW": "4"}, {"CMLPL_PAIR16": "1"},
            {"CMLPL_PAIR_TALL": "0"}, {"CMLPL_PAIR_TALL": "1"}, {"CMLPL_PAIR_TALL": "0", "CMLPL_PAIR_WIDE": "1"}]
    for env in envs:
        switches(env)
        for K in (32, 33, 48, 64):
            for nunl, Q in ((16, 256), (16, 4096), (100, 4096), (200, 8192)):
                p = read_plan(K, 16, nunl, Q, True)
                if K > 32:
                    assert p.kernel in BOTH_EPILOGUES, (env, K, nunl, Q, p)
                _covers(p, nunl, Q)


def test_arguments_the_loss_block_refuses_are_refused(switches):
    import ctypes as C
    lib = _lib.load()
    out = (C.c_int * 9)()
    ask = lambda K, sh, Q: lib.cmlpl_debug_loss_plan(C.byref(_lib.Shape(60, 20, 20, 103, K)), C.byref(_lib.Shard(*sh)), Q, 1, out)
    assert ask(9, (16, 16, 0, 16, 0, 16), 32) == 0
    assert ask(9, (16, 16, 0, 16, 0, 16), 31) == -1              # banks narrower than the batch
    assert ask(9, (16, 2049, 0, 16, 0, 16), 8192) == -1          # btu <= 2048
    assert ask(9, (16, 16, 0, 16, 8, 16), 64) == -1              # the shard's rows past the batch
    assert ask(65, (16, 16, 0, 16, 0, 16), 64) == -2 and ask(0, (16, 16, 0, 16, 0, 16), 64) == -2
    assert lib.cmlpl_debug_loss_plan(C.byref(_lib.Shape(60, 20, 20, 103, 9)), None, 64, 1, out) == -1
