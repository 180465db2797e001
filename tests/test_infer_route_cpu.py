"""CPU: which route whole-scene inference takes for a window shape, and which shapes it takes at all, against the
inference-envelope table (tests/infer_cases.py).

`infer_fused` asks the library's router (route_infer in conv3x3.hip, through cmlpl_infer_workspace_bytes),
`infer_supported` adds the by-patches route: the general forward's workspace AND the cut of one window
(cmlpl_patches_fit, answered from the launchers' own LDS sizes).  Host arithmetic only -- until the query existed
`infer_supported` said yes to windows cmlpl_extract_patches refuses (103 channels at 20 x 20), and the refusal came at
the end of a training run.  The GPU side of the same table is tests/test_gpu_infer_envelope.py."""
import ctypes as C
import os

import pytest

from cmlpl_amd import _lib
from oracle import cmlpl_oracle as O
from tests.infer_cases import CASES, CUT_FITS, CUT_TOO_LARGE, FORCED_BY_PATCHES, FORCED_REFUSED, BY_ID, FUSED4, FUSED8, PATCHES

SWITCHES = ("CMLPL_CONV3_S", "CMLPL_FUSE_TAIL", "CMLPL_FUSE_CONV0", "CMLPL_FUSE_BIG")
LDS_MAX = 160 * 1024


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


def _route(shape):
    """the table's word for what the library does with a window shape"""
    from cmlpl_amd.infer import infer_fused
    if not infer_fused(shape):
        return PATCHES
    return FUSED4 if shape.H * shape.W <= 128 else FUSED8          # (route_infer: the eight-tile kernels from 129 pixels)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_case_takes_the_route_the_table_names(case, switches):
    from cmlpl_amd.infer import infer_supported
    s = O.NetShape(*case.shape)
    assert _route(s) == case.route, case.why
    assert infer_supported(s)
    assert case.rows >= s.H // 2 and case.cols >= s.W // 2          # (a scene the launcher takes)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_no_case_is_fused_without_the_fused_tail(case, switches):
    from cmlpl_amd.infer import infer_fused, infer_supported
    switches({"CMLPL_FUSE_TAIL": "0"})
    s = O.NetShape(*case.shape)
    assert not infer_fused(s)
    assert infer_supported(s) == (case.id != FORCED_REFUSED)          # 256 channels at 14 x 14: no cut takes the window
    if case.id in FORCED_BY_PATCHES:
        assert infer_supported(s)


def test_the_table_covers_what_it_says():
    """the table itself: every route, both pass boundaries on both fused kernels, and the scene limit both ways"""
    by = lambda r: [c for c in CASES if c.route == r]
    for r in (FUSED4, FUSED8):
        cs = {c.shape[0] for c in by(r)}
        assert 112 in cs and 113 in cs and any(c > 224 for c in cs), r
    assert {c.shape[1] for c in by(FUSED4)} >= {8, 9, 10, 11} and {c.shape[1] for c in by(FUSED8)} >= {12, 13, 14, 15}
    assert {c.shape[1] for c in by(PATCHES)} >= {4, 7, 16, 20}
    t = BY_ID["tiny-11"]
    assert (t.rows, t.cols) == (t.shape[1] // 2, t.shape[1] // 2)
    assert BY_ID["tiny-15"].rows == 7 and BY_ID["tiny-8"].cols == 4
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("shape", CUT_TOO_LARGE, ids=lambda s: "x".join(map(str, s)))
def test_a_window_no_cut_takes_is_not_supported(shape, switches):
    from cmlpl_amd.infer import infer_fused, infer_supported
    lib = _lib.load()
    s = O.NetShape(*shape)
    cs = _lib.Shape(*shape)
    assert lib.cmlpl_workspace_bytes(C.byref(cs), 1, 8, 8) > 0       # the general forward itself takes the window:
    assert not infer_fused(s) and not infer_supported(s)             # what used to be the whole answer
    assert lib.cmlpl_patches_fit(s.C, s.H) == 0


@pytest.mark.parametrize("shape", CUT_FITS, ids=lambda s: "x".join(map(str, s)))
def test_a_window_the_cuts_take_is_supported(shape, switches):
    from cmlpl_amd.infer import infer_supported
    s = O.NetShape(*shape)
    assert infer_supported(s) and _lib.load().cmlpl_patches_fit(s.C, s.H) == 3


def test_patches_fit_is_the_launchers_arithmetic():
    """cmlpl_patches_fit over the whole (C, w) envelope against the LDS sizes augment.hip / tta.hip document: bit 0 the
    clean cut's padded tile (odd C: rows of w C floats rounded up to 16 bytes; even C: C + 1 floats per pixel), bit 1 the
    view cut's (C | 1 floats per pixel); nothing for an empty window"""
    lib = _lib.load()
    for w in range(1, 25):
        for ch in list(range(1, 260)) + [1000, 65536]:
            clean = w * ((w * ch + 3) & ~3) * 4 if ch & 1 else w * w * (ch + 1) * 4
            view = w * w * (ch | 1) * 4
            assert lib.cmlpl_patches_fit(ch, w) == (clean <= LDS_MAX) + 2 * (view <= LDS_MAX), (ch, w)
    for ch, w in ((0, 8), (8, 0), (-1, 8), (8, -3), (1 << 30, 1 << 15), (65537, 1)):
        assert lib.cmlpl_patches_fit(ch, w) == 0
    # the boundary the reference's own configuration meets: PaviaU's 103 raw bands under its 20 x 20 window
    assert lib.cmlpl_patches_fit(101, 20) == 3 and lib.cmlpl_patches_fit(102, 20) == 0 and lib.cmlpl_patches_fit(103, 20) == 0
