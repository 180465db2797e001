"""CPU: the C surface of the schedule / weight-decay / clipping options -- new symbols exported and bound, the ABI still 6,
no existing record moved (sizes and offsets against a compiled C program), the definition in the header where the other
after-ABI-6 sections stand, and the argument checks that run in front of any device call (no GPU: no pointer is followed).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cmlpl_grad_norm_partials_bytes", "cmlpl_grad_norm", "cmlpl_adam_step_opt", "cmlpl_train_step_opt",
       "cmlpl_step_graph_create_opt", "cmlpl_dyn_adam_opt")
FAKE = 0x10000
# what tests/test_spatial_host.py and tests/test_cube_feed_abi.py hold the records to, restated
PINNED = {"cmlpl_step_io": (296, {"d_scalars": 144, "adam_t": 200, "apply_update": 224, "reserved": 228, "d_dyn_table": 248,
                                  "d_dyn_cursor": 256, "d_cube": 264, "d_unl_pix": 288}),
          "cmlpl_batch": (104, {"d_lab_idx": 56, "d_cube": 72}),
          "cmlpl_dyn": (64, {"hist_row": 48, "adam_step_size": 52, "adam_bc2_sqrt": 56, "reserved": 60})}


def test_new_symbols_are_exported_and_the_abi_is_still_6():
    from cmlpl_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert _lib.ABI_VERSION == 6 and lib.cmlpl_abi_version() == 6
    nbytes = lib.cmlpl_grad_norm_partials_bytes()
    assert 0 < nbytes <= 2 * 64 * 8 and nbytes % 8 == 0          # at most 64 fp64 partials per network


def test_no_record_has_moved(tmp_path):
    from cmlpl_amd import _lib
    recs = {"cmlpl_step_io": _lib.StepIO, "cmlpl_batch": _lib.Batch, "cmlpl_dyn": _lib.Dyn, "cmlpl_optim": _lib.Optim}
    for n, (size, offs) in PINNED.items():
        assert C.sizeof(recs[n]) == size, (n, C.sizeof(recs[n]))
        for f, o in offs.items():
            assert getattr(recs[n], f).offset == o, (n, f)
    assert dict(_lib.Dyn._fields_)["reserved"] is C.c_int32
    assert dict((f[0], f[1:]) for f in _lib.DYN_DTYPE)["reserved"] == ("<i4",)
    assert np.dtype(_lib.DYN_DTYPE).itemsize == 64 and np.dtype(_lib.DYN_DTYPE).fields["reserved"][1] == 60
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [(n, f) for n, (_, offs) in PINNED.items() for f in offs] + \
             [("cmlpl_optim", f) for f in ("max_norm", "weight_decay", "d_norms", "d_partials")]
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


def test_header_carries_the_definition_under_the_no_bump_heading():
    src = open(os.path.join(ROOT, "include", "cmlpl.h")).read()
    assert "#define CMLPL_ABI_VERSION 6" in src
    head = src.index("ADDED AFTER ABI 6 WITHOUT A VERSION BUMP")
    at = src.index("THE DEFINITION OF A CLIPPED, DECAYED ADAM STEP")
    assert at > head
    section = src[at:]
    for phrase in ("(double)g * (double)g", "1e-6f", "max_norm == 0", "keep = (float)(1.0 - (double)lr_t", "reserved",
                   "all-zero bits", "do NOT count", "no floating-point atomics"):
        assert phrase in section, phrase
    for name in NEW:
        assert name + "(" in section, name
    assert "int32_t reserved;" in src[src.index("typedef struct cmlpl_dyn"):src.index("} cmlpl_dyn;")]


def _hp(lr=5e-4):
    from cmlpl_amd import _lib
    return _lib.HParams(lr, 0.9, 0.999, 1e-8, 0.3, 0.95, 0.5, 0.8, 0.5, 4.0, 0.8, 0.3)


def test_dyn_adam_opt_is_dyn_adam_and_the_decay_factor():
    from cmlpl_amd import _lib
    lib = _lib.load()
    a, b, k, a0, b0 = (C.c_float() for _ in range(5))
    for t in (1, 2, 7, 1580):
        for wd in (0.0, 0.05, 3.0):
            hp = _hp()
            assert lib.cmlpl_dyn_adam_opt(C.byref(hp), t, wd, C.byref(a), C.byref(b), C.byref(k)) == 0
            assert lib.cmlpl_dyn_adam(C.byref(hp), t, C.byref(a0), C.byref(b0)) == 0
            assert (a.value, b.value) == (a0.value, b0.value)
            want = np.float32(1.0 - float(np.float32(5e-4)) * float(np.float32(wd)))
            assert np.float32(k.value).tobytes() == want.tobytes(), (t, wd)
            assert np.float32(k.value).view(np.int32) != 0               # never the bits that mean "off"
    assert k.value < 1.0
    assert lib.cmlpl_dyn_adam_opt(C.byref(_hp(0.5)), 1, 2.0, C.byref(a), C.byref(b), C.byref(k)) == -1   # keep == 0.0f
    assert lib.cmlpl_dyn_adam_opt(C.byref(_hp()), 1, -1.0, C.byref(a), C.byref(b), C.byref(k)) == -1
    assert lib.cmlpl_dyn_adam_opt(C.byref(_hp()), 1, float("nan"), C.byref(a), C.byref(b), C.byref(k)) == -1
    assert lib.cmlpl_dyn_adam_opt(C.byref(_hp()), 0, 0.0, C.byref(a), C.byref(b), C.byref(k)) == -1
    assert lib.cmlpl_dyn_adam_opt(C.byref(_hp()), 1, 0.0, C.byref(a), C.byref(b), None) == -1


def test_malformed_options_are_argument_errors():
    from cmlpl_amd import _lib
    lib = _lib.load()
    cs = _lib.Shape(103, 11, 11, 103, 9)
    P = int(_lib.layout(cs).param_total)
    p = C.c_void_p(FAKE)

    def adam(opt, hp=None, stride=P):
        hp = hp or _hp()
        return lib.cmlpl_adam_step_opt(C.byref(cs), 2, p, P, p, stride, p, p, 1, C.byref(hp), None, C.byref(opt), None)
    assert adam(_lib.Optim(-1.0, 0.0, None, FAKE)) == -1
    assert adam(_lib.Optim(float("nan"), 0.0, None, FAKE)) == -1
    assert adam(_lib.Optim(float("inf"), 0.0, None, FAKE)) == -1
    assert adam(_lib.Optim(0.0, -0.1, None, FAKE)) == -1
    assert adam(_lib.Optim(1.0, 0.0, None, None)) == -1                 # clipping needs the partials
    assert adam(_lib.Optim(0.0, 0.0, FAKE, None)) == -1                 # and so does the norms row
    assert adam(_lib.Optim(1.0, 0.0, None, FAKE + 4)) == -1             # fp64 partials: 8-byte aligned
    assert adam(_lib.Optim(1.0, 0.0, FAKE + 2, FAKE)) == -1
    assert adam(_lib.Optim(0.0, 2.0, None, None), hp=_hp(0.5)) == -1    # keep == 0.0f
    assert adam(_lib.Optim(1.0, 0.0, None, FAKE), stride=P - 4) == -1
    norm = lambda nets, stride, mx, part, out: lib.cmlpl_grad_norm(C.byref(cs), nets, p, stride, mx, part, out, None)
    assert norm(0, P, 1.0, p, p) == -1 and norm(3, P, 1.0, p, p) == -1
    assert norm(2, P - 4, 1.0, p, p) == -1
    assert norm(2, P, -1.0, p, p) == -1 and norm(2, P, float("nan"), p, p) == -1
    assert norm(2, P, 1.0, None, p) == -1 and norm(2, P, 1.0, p, None) == -1
    assert lib.cmlpl_grad_norm(C.byref(_lib.Shape(60, 3, 3, 103, 9)), 2, p, P, 1.0, p, p, None) == -2
    # the step: the options are checked with the rest, in front of the first launch
    io = _lib.StepIO()
    for k in ("d_xpl", "d_xpu", "d_xl", "d_labels", "d_xu", "d_params", "d_m", "d_v", "d_grads", "d_packed", "d_scalars",
              "d_logits", "d_feat", "d_workspace"):
        setattr(io, k, FAKE)
    for i in range(2):
        io.banks.d_feats[i] = io.banks.d_probs[i] = FAKE
    io.banks.Q, io.bt, io.btu, io.workspace_bytes, io.adam_t, io.apply_update = 160, 8, 8, 1 << 40, 1, 1
    step = lambda opt, hp: lib.cmlpl_train_step_opt(C.byref(cs), C.byref(hp), C.byref(io), C.byref(opt), None)
    assert step(_lib.Optim(-1.0, 0.0, None, FAKE), _hp()) == -1
    assert step(_lib.Optim(1.0, 0.0, None, None), _hp()) == -1
    assert step(_lib.Optim(0.0, 2.0, None, None), _hp(0.5)) == -1
    handle = C.c_void_p()
    assert lib.cmlpl_step_graph_create_opt(C.byref(cs), C.byref(_hp()), C.byref(io), C.byref(_lib.Optim(1.0, 0.0, None, FAKE)),
                                           None, C.byref(handle)) == -1          # no table: as cmlpl_step_graph_create
