"""GPU: the gradient fold that applies Adam itself (csrc/conv0.hip: reduce_gemm_adam_kernel) against
the two launches it replaces (CMLPL_FUSE_ADAM=0: reduce_gemm_kernel + adam_kernel).  The fused launch changes no
arithmetic and no summation order, so nothing here has a tolerance: parameters, m, v, gradients, the whole packed block
with its flag words, logits and the logged row are compared as BYTES after one step and after three (three make the
packed copies the fused launch wrote feed the next forward).

Shapes are chosen for the new indexing, not for the workload: an 11 x 11 window with C = bands = 7 (per-sample route;
conv0's partial has ragged rows, C * HW is no multiple of 4), a 20 x 20 window with C = 6 (general path), C = bands = 40
with K = 3 (several conv0 reduce blocks; a classifier tile narrower than 32, one pad float behind its bias); batches of
3 + 2 (G below 32: the slice loop runs once, a partial GEMM row tail) and 20 + 17 (it iterates); both methods.
"""
import ctypes as C
import os

import pytest
import torch

from oracle import cmlpl_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"w11c7": O.NetShape(7, 11, 11, 7, 9), "w20c6": O.NetShape(6, 20, 20, 6, 9), "w11c40k3": O.NetShape(40, 11, 11, 40, 3)}
BATCHES = {"3+2": (3, 2), "20+17": (20, 17)}
FIELDS = ("params", "m", "v", "grads", "packed", "logits", "scalars")
_params = {}      # (shape name, seed) -> closed-form parameters, formed once


class _NoNormsRow:
    """the engine's library with the options record of every step stripped of its norms row: weight decay alone"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def cmlpl_train_step_opt(self, cs, hp, io, opt, stream):
        opt._obj.d_norms = None
        return self._lib.cmlpl_train_step_opt(cs, hp, io, opt, stream)


def _switch(value):
    from cmlpl_amd import _lib
    if value is None:
        os.environ.pop("CMLPL_FUSE_ADAM", None)
    else:
        os.environ["CMLPL_FUSE_ADAM"] = value
    _lib.load().cmlpl_debug_reload_switches()


def _snapshot(eng):
    torch.cuda.synchronize()
    got = {"params": eng.params, "m": eng.m, "v": eng.v, "grads": eng.grads, "packed": eng.packed, "logits": eng.logits,
           "scalars": eng.scalar_hist}
    return {k: t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes() for k, t in got.items()}


def _run(name, batch, fuse, method="cmlpl", steps=(1, 3), optim=None, strip_norms=False, tweak=None, after_pack=None,
         apply_update=True, counts=None):
    """steps from one common state with CMLPL_FUSE_ADAM = fuse -> {step count: {field: bytes}} (+ the launch counts)"""
    from cmlpl_amd import HyperParams, NetShape, TrainEngine, _lib
    shape = SHAPES[name]
    bt, btu = BATCHES[batch]
    old = os.environ.get("CMLPL_FUSE_ADAM")
    _switch(fuse)
    try:
        eng = TrainEngine(NetShape(shape.C, shape.H, shape.W, shape.bands, shape.K), bt, btu, HyperParams(), device=DEV,
                          seed=3, method=method, optim=optim)
        if strip_norms:
            eng.lib = _NoNormsRow(eng.lib)
        for net in range(2):
            key = (name, 9 + net)
            if key not in _params:
                _params[key] = O.closed_form_params(shape, 9 + net)
            sd = {k: v.clone() for k, v in _params[key].items()}
            if tweak is not None:
                tweak(sd)
            eng.load_state_dict(net, sd)
        if after_pack is not None:
            eng._ensure_packed(C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
            after_pack(eng)
        out = {}
        d = lambda t: t.to(DEV)
        nk = len(_lib.KERNEL_NAMES)
        ms, cnt = (C.c_double * nk)(), (C.c_int64 * nk)()
        if counts is not None:
            _lib.check("cmlpl_timing_begin", eng.lib.cmlpl_timing_begin(0xFFFFFFFF, 64))
        try:
            for s in range(max(steps)):
                b = O.synthetic_batch(shape, bt, btu, 41 + s)
                eng.step(d(b["XPl"]), d(b["Xl"]), d(b["Y"]), d(b["XPu"]), d(b["Xu"]), 1, s, apply_update=apply_update)
                if s + 1 in steps:
                    out[s + 1] = _snapshot(eng)
        finally:
            if counts is not None:
                rc = eng.lib.cmlpl_timing_end(ms, cnt)
        if counts is not None:
            _lib.check("cmlpl_timing_end", rc)
            counts.update({k: int(cnt[i]) for i, k in enumerate(_lib.KERNEL_NAMES)})
        return out
    finally:
        _switch(old)


def _same(a, b, what):
    for step in a:
        for f in FIELDS:
            assert a[step][f] == b[step][f], f"{what}: `{f}` differs after {step} step(s)"


@pytest.mark.parametrize("method", ["cmlpl", "cps"])
@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fused_step_equals_the_two_launches_byte_for_byte(name, batch, method):
    fused = _run(name, batch, "1", method=method)
    two = _run(name, batch, "0", method=method)
    _same(fused, two, f"{name} {batch} {method}")
    assert fused[1]["params"] != fused[3]["params"]                  # (the steps did move the parameters)


def test_the_default_is_the_fused_launch_and_it_leaves_the_adam_slot_empty():
    c_default, c_on, c_off = {}, {}, {}
    a = _run("w11c7", "3+2", None, steps=(1,), counts=c_default)
    b = _run("w11c7", "3+2", "1", steps=(1,), counts=c_on)
    c = _run("w11c7", "3+2", "0", steps=(1,), counts=c_off)
    assert c_default["adam"] == 0 and c_on["adam"] == 0 and c_off["adam"] == 1
    assert c_default["conv1_wred"] == 1 and c_on["conv1_wred"] == 1 and c_off["conv1_wred"] == 1
    _same(a, b, "default against CMLPL_FUSE_ADAM=1")
    _same(a, c, "default against CMLPL_FUSE_ADAM=0")


def test_weight_decay_without_a_norms_row_takes_the_fused_launch():
    from cmlpl_amd.optim import OptimConfig
    opt = OptimConfig(weight_decay=0.05)
    c_on, c_off = {}, {}
    fused = _run("w11c40k3", "20+17", "1", optim=opt, strip_norms=True, counts=c_on)
    two = _run("w11c40k3", "20+17", "0", optim=opt, strip_norms=True, counts=c_off)
    assert c_on["adam"] == 0 and c_off["adam"] == 3
    _same(fused, two, "weight decay")
    plain = _run("w11c40k3", "20+17", "1", steps=(3,))
    assert plain[3]["params"] != fused[3]["params"]                  # (the decay is applied)


def test_clipping_and_a_step_without_update_keep_the_two_launches():
    from cmlpl_amd.optim import OptimConfig
    clip, none = {}, {}
    a = _run("w11c7", "3+2", "1", steps=(1,), optim=OptimConfig(clip_grad=1.0), counts=clip)
    b = _run("w11c7", "3+2", "0", steps=(1,), optim=OptimConfig(clip_grad=1.0))
    assert clip["adam"] == 1 and clip["conv1_wred"] == 1
    _same(a, b, "clipped step")
    first = _run("w11c7", "3+2", "1", steps=(1,), apply_update=False, counts=none)
    second = _run("w11c7", "3+2", "0", steps=(1,), apply_update=False)
    assert none["adam"] == 0
    _same(first, second, "step without update")
    zeros = bytes(len(first[1]["m"]))
    assert first[1]["m"] == zeros and first[1]["v"] == zeros          # nothing was updated


def _flags(snap, eng_shape):
    from cmlpl_amd import _lib
    lay = _lib.layout(_lib.Shape(eng_shape.C, eng_shape.H, eng_shape.W, eng_shape.bands, eng_shape.K))
    words = torch.frombuffer(bytearray(snap["packed"]), dtype=torch.int32).view(2, -1)
    return words[:, int(lay.packed_total) - 16].tolist()


def test_a_weight_at_8_keeps_the_flag_raised_on_both_paths():
    def tweak(sd):
        sd["conv1.weight"][3, 5, 1, 1] = 8.0                           # 8 * 2^13 > 65504
    fused = _run("w11c7", "20+17", "1", tweak=tweak)
    two = _run("w11c7", "20+17", "0", tweak=tweak)
    for step in (1, 3):
        assert _flags(fused[step], SHAPES["w11c7"]) == [1, 1] and _flags(two[step], SHAPES["w11c7"]) == [1, 1]
    _same(fused, two, "weight at 8.0")                                # equal logits: the forward took the three-piece loop


def test_the_fused_launch_raises_a_cleared_flag_itself():
    """a weight that fp16 still holds at the packing scale (7.95 * 2^13 = 65126 < 65504) but that lies beyond the range
    bound of 65000: the full pack raises the flag, the test clears it, and the update's own packing must raise it again"""
    def tweak(sd):
        sd["conv1.weight"][3, 5, 1, 1] = 7.95
        sd["conv2.weight"][60, 63, 2, 0] = -7.95

    def clear(eng):
        assert eng._flag_words()[:, 0].tolist() == [1, 1]
        eng._flag_words().zero_()
    fused = _run("w11c7", "3+2", "1", tweak=tweak, after_pack=clear)
    two = _run("w11c7", "3+2", "0", tweak=tweak, after_pack=clear)
    assert _flags(fused[1], SHAPES["w11c7"]) == [1, 1] and _flags(two[1], SHAPES["w11c7"]) == [1, 1]
    _same(fused, two, "cleared flag")
