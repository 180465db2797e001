"""CPU: ABI 6 -- the cube-fed batch fields of cmlpl_batch / cmlpl_step_io (and of the cmlpl_batch that cmlpl_dist_io
embeds).  The ctypes records must have the header's sizes and field offsets (checked against a compiled C program), and
every malformed cube-fed batch must come back as CMLPL_E_ARG / CMLPL_E_SHAPE from the argument checks, which run in
front of any device call (so these calls need no GPU: the pointers are never followed)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE = -1, -2
FAKE = 0x10000          # a non-null "device pointer" (never dereferenced: the calls return from their argument checks)


def test_abi_version_is_6():
    from cmlpl_amd import _lib
    assert _lib.ABI_VERSION == 6 and _lib.load().cmlpl_abi_version() == 6


def test_ctypes_records_match_the_header(tmp_path):
    from cmlpl_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    recs = {"cmlpl_batch": _lib.Batch, "cmlpl_step_io": _lib.StepIO, "cmlpl_dist_io": _lib.DistIO, "cmlpl_shard": _lib.Shard,
            "cmlpl_dyn": _lib.Dyn, "cmlpl_banks": _lib.Banks, "cmlpl_gathered": _lib.Gathered}
    fields = [("cmlpl_batch", f) for f in ("d_lab_idx", "d_cube", "cube_rows", "cube_cols", "d_lab_pix", "d_unl_pix")] + \
             [("cmlpl_step_io", f) for f in ("d_dyn_cursor", "d_cube", "cube_rows", "cube_cols", "d_lab_pix", "d_unl_pix")] + \
             [("cmlpl_dist_io", f) for f in ("batch", "shard", "gathered", "banks", "d_params", "seed", "d_dyn_cursor")]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cmlpl.h"', 'int main(void) {']
    src += [f'  printf("{n} %zu\\n", sizeof({n}));' for n in recs]
    src += [f'  printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for n, f in fields]
    src += ['  return 0;', '}']
    (tmp_path / "sizes.c").write_text("\n".join(src))
    exe = str(tmp_path / "sizes")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "sizes.c"), "-o", exe], check=True)
    out = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for n, rec in recs.items():
        assert C.sizeof(rec) == int(out[n]), (n, C.sizeof(rec), out[n])
    for n, f in fields:
        assert getattr(recs[n], f).offset == int(out[f"{n}.{f}"]), (n, f)


def _forward(batch, shape=(103, 11, 11, 103, 9), spatial=False):
    from cmlpl_amd import _lib
    lib = _lib.load()
    cs = _lib.Shape(*shape)
    hp = _lib.HParams(5e-4, 0.9, 0.999, 1e-8, 0.3, 0.95, 0.5, 0.8, 0.5, 4.0, 0.8, 0.3)
    p = C.c_void_p(FAKE)
    if spatial:
        return lib.cmlpl_forward_spatial(C.byref(cs), C.byref(hp), C.byref(batch), None, p, p, None, 1, 1, 0, p, p, 1 << 40, None)
    return lib.cmlpl_forward(C.byref(cs), C.byref(hp), C.byref(batch), None, p, p, None, 1, 1, 0, p, p, None, p, 1 << 40, None)


def _cube_batch(**kw):
    from cmlpl_amd import _lib
    b = _lib.Batch()
    b.d_xl = b.d_xu = b.d_labels = FAKE
    b.bt, b.btu = 8, 8
    b.d_cube, b.cube_rows, b.cube_cols, b.d_lab_pix, b.d_unl_pix = FAKE, 32, 40, FAKE, FAKE
    for k, v in kw.items():
        setattr(b, k, v)
    return b


@pytest.mark.parametrize("spatial", [False, True])
def test_malformed_cube_batches_are_argument_errors(spatial):
    assert _forward(_cube_batch(d_xpl=FAKE), spatial=spatial) == E_ARG                 # the cube together with patch pointers
    assert _forward(_cube_batch(d_xpu=FAKE), spatial=spatial) == E_ARG
    assert _forward(_cube_batch(d_lab_pix=None), spatial=spatial) == E_ARG             # a pixel list missing
    assert _forward(_cube_batch(d_unl_pix=None), spatial=spatial) == E_ARG
    assert _forward(_cube_batch(cube_rows=0), spatial=spatial) == E_ARG
    assert _forward(_cube_batch(cube_rows=10), spatial=spatial) == E_SHAPE             # the scene smaller than the window
    assert _forward(_cube_batch(cube_cols=10), spatial=spatial) == E_SHAPE
    assert _forward(_cube_batch(), shape=(103, 11, 12, 103, 9), spatial=spatial) == E_SHAPE     # H != W
    assert _forward(_cube_batch(cube_rows=64, cube_cols=64), shape=(256, 16, 16, 103, 9), spatial=spatial) == E_SHAPE  # tile > LDS
    # and the split-fed batch keeps its own check: no cube, no patch pointers
    assert _forward(_cube_batch(d_cube=None), spatial=spatial) == E_ARG


def test_malformed_cube_step_is_an_argument_error():
    """the same checks through cmlpl_train_step's cmlpl_step_io"""
    from cmlpl_amd import _lib
    lib = _lib.load()
    cs = _lib.Shape(103, 11, 11, 103, 9)
    hp = _lib.HParams(5e-4, 0.9, 0.999, 1e-8, 0.3, 0.95, 0.5, 0.8, 0.5, 4.0, 0.8, 0.3)

    def io(**kw):
        r = _lib.StepIO()
        for k in ("d_xl", "d_labels", "d_xu", "d_params", "d_m", "d_v", "d_grads", "d_packed", "d_scalars", "d_logits",
                  "d_feat", "d_workspace", "d_cube", "d_lab_pix", "d_unl_pix"):
            setattr(r, k, FAKE)
        for i in range(2):
            r.banks.d_feats[i] = r.banks.d_probs[i] = FAKE
        r.banks.Q, r.bt, r.btu, r.workspace_bytes, r.adam_t, r.apply_update = 160, 8, 8, 1 << 40, 1, 1
        r.cube_rows, r.cube_cols = 32, 40
        for k, v in kw.items():
            setattr(r, k, v)
        return r
    step = lambda r: lib.cmlpl_train_step(C.byref(cs), C.byref(hp), C.byref(r), None)
    assert step(io(d_xpl=FAKE)) == E_ARG
    assert step(io(d_unl_pix=None)) == E_ARG
    assert step(io(cube_cols=5)) == E_SHAPE
    assert step(io(d_cube=None)) == E_ARG
