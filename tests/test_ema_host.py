"""CPU: the EMA teacher's plumbing -- the fixture of the reference's own ``WeightEMA_BN`` (tests/golden/ema/*.npz, written
by tests/golden/make_golden_ema.py) against the three-rounding formula restated here in numpy float32, the export and
its argument checks (in front of any launch: no GPU), the command lines, the checkpoint identity and the run record."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ema")
FLOAT_KEYS = ("l1.weight", "l1.bias", "l2.weight", "l2.bias", "wide")
E_ARG = -1
FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer" (never dereferenced)


def ema_formula(src, ema, alpha):
    """ema' = fl(fl(src * oma) + fl(ema * a)), a = float32(alpha), oma = float32(1.0 - alpha) with the difference taken
    in DOUBLE: numpy's float32 products and sum round once each"""
    a, oma = np.float32(alpha), np.float32(1.0 - float(alpha))
    p = (src.astype(np.float32) * oma).astype(np.float32)
    q = (ema.astype(np.float32) * a).astype(np.float32)
    return (p + q).astype(np.float32)


def ema_contracted(src, ema, alpha):
    """what an FMA makes of it: fl(src * oma + fl(ema * a)), the first product exact (fp64 holds a product of two fp32
    exactly; the sum's double rounding is far below what this is used to show)"""
    a, oma = np.float32(alpha), np.float32(1.0 - float(alpha))
    q = (ema.astype(np.float32) * a).astype(np.float32)
    return (src.astype(np.float64) * np.float64(oma) + q.astype(np.float64)).astype(np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def fixtures():
    return [(tag, np.load(os.path.join(GOLDEN, tag + ".npz"))) for tag in ("a95", "a999")]


def test_fixture_is_what_the_generator_says():
    for tag, z in fixtures():
        assert float(z["alpha"][0]) == {"a95": 0.95, "a999": 0.999}[tag] and int(z["calls"][0]) == 4
        assert z["ens0.wide"].shape == (4099,) and z["ens0.l1.weight"].shape == (5, 7) and z["ens0.l2.weight"].shape == (3, 5)
        mag = np.abs(z["ens0.wide"])
        assert mag.min() < 1e-5 and mag.max() > 1e2            # the magnitudes span what the generator drew
        assert os.path.getsize(os.path.join(GOLDEN, tag + ".npz")) < 1 << 20


def test_three_rounding_formula_equals_the_reference_bit_for_bit():
    for tag, z in fixtures():
        alpha, calls = float(z["alpha"][0]), int(z["calls"][0])
        for c in range(1, calls + 1):
            for k in FLOAT_KEYS:
                got = ema_formula(z[f"base{c}.{k}"], z[f"ens{c - 1}.{k}"], alpha)
                want = z[f"ens{c}.{k}"]
                bad = int((bits(got) != bits(want)).sum())
                print(tag, c, k, "elements that differ:", bad, "of", want.size)
                assert bad == 0, (tag, c, k)
            # the integer entry: the fp32 expression, cast back by load_state_dict's copy (towards zero)
            b, e = z[f"base{c}.count"], z[f"ens{c - 1}.count"]
            want = np.float32(np.float32(b) * np.float32(1.0 - alpha) + np.float32(e) * np.float32(alpha))
            assert int(z[f"ens{c}.count"]) == int(want), (tag, c)


def test_contracted_formula_does_not_match_the_fixture():
    """the fixture can tell the two apart: an FMA in the kernel would show"""
    for tag, z in fixtures():
        alpha = float(z["alpha"][0])
        got = ema_contracted(z["base1.wide"], z["ens0.wide"], alpha)
        frac = float((bits(got) != bits(z["ens1.wide"])).mean())
        print(tag, "contracted form: share of elements that differ = %.4f" % frac)
        assert frac > 0.01, (tag, frac)


def test_one_minus_alpha_from_the_float_argument_does_not_match_either():
    """why the C entry point takes alpha as a double: 1.0f - (float)alpha is not (float)(1.0 - alpha)"""
    for tag, z in fixtures():
        alpha = float(z["alpha"][0])
        a = np.float32(alpha)
        oma = np.float32(1.0 - float(a))
        assert oma != np.float32(1.0 - alpha)
        got = ((z["base1.wide"] * oma).astype(np.float32) + (z["ens0.wide"] * a).astype(np.float32)).astype(np.float32)
        assert float((bits(got) != bits(z["ens1.wide"])).mean()) > 0.1


def _lib_loaded():
    from cmlpl_amd import _lib, build_ext
    if build_ext.needs_build():
        build_ext.build(verbose=False)
    return _lib, _lib.load()


def test_export_header_binding_and_version():
    _lib, lib = _lib_loaded()
    assert "cmlpl_ema_update" in _lib.EXPORTS and hasattr(lib, "cmlpl_ema_update")
    assert _lib.ABI_VERSION == 6 and lib.cmlpl_abi_version() == 6           # added after ABI 6, no bump
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cmlpl.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+cmlpl_ema_update\s*\(([^)]*)\)\s*;", code)
    assert m
    params = [" ".join(p.split()[:-1]) + "*" * p.split()[-1].count("*") for p in m.group(1).split(",")]
    assert params == ["const float*", "float*", "int64_t", "double", "void*"], params
    assert list(lib.cmlpl_ema_update.argtypes) == [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]
    assert lib.cmlpl_ema_update.restype is C.c_int
    from cmlpl_amd import build_ext
    assert "ema.hip" in build_ext.SOURCES
    # no record changed size, the step's record least of all: the update is a call of its own behind the step
    assert C.sizeof(_lib.StepIO) == 296 and C.sizeof(_lib.Dyn) == 64


def test_argument_checks_return_e_arg_before_any_launch():
    _lib, lib = _lib_loaded()
    f = lib.cmlpl_ema_update
    assert f(None, None, 0, 0.95, None) == 0                     # count == 0: nothing to do, whatever the pointers
    assert f(FAKE, FAKE, 0, 0.95, None) == 0
    assert f(None, FAKE, 4, 0.95, None) == E_ARG
    assert f(FAKE, None, 4, 0.95, None) == E_ARG
    assert f(FAKE, FAKE, -1, 0.95, None) == E_ARG
    for bad in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert f(FAKE, FAKE, 4, bad, None) == E_ARG, bad
        assert f(FAKE, FAKE, 0, bad, None) == E_ARG, bad
    assert f(FAKE + 2, FAKE, 4, 0.95, None) == E_ARG             # not a float's alignment
    assert f(FAKE, FAKE + 1, 4, 0.95, None) == E_ARG


def test_parser_and_run_record():
    import train
    from cmlpl_amd import HyperParams
    p = train.build_parser()
    a0 = p.parse_args(["--synthetic", "B2"])
    a1 = p.parse_args(["--synthetic", "B2", "--ema"])
    a2 = p.parse_args(["--synthetic", "B2", "--ema", "--teacher_alpha", "0.9"])
    assert a0.ema is False and a1.ema is True and a1.teacher_alpha == 0.95 and a2.teacher_alpha == 0.9
    r0, r1, r2 = (train.run_record(a, HyperParams(), train.SYNTH["B2"], False) for a in (a0, a1, a2))
    # without --ema the record is what it was: the flag (and the ignored --teacher_alpha) leave no trace
    assert "ema" not in r0 and "teacher_alpha" not in r0
    assert r0 == train.run_record(p.parse_args(["--synthetic", "B2", "--teacher_alpha", "0.5"]), HyperParams(),
                                  train.SYNTH["B2"], False)
    assert r1["ema"] is True and r1["teacher_alpha"] == 0.95
    assert {k: v for k, v in r1.items() if k not in ("ema", "teacher_alpha")} == r0
    # --resume refuses both ways, and another coefficient
    assert train.run_differences(r0, r0) == [] and train.run_differences(r1, r1) == []
    for saved, mine in ((r0, r1), (r1, r0), (r1, r2)):
        d = train.run_differences(saved, mine)
        assert d and any(s.startswith(("ema:", "teacher_alpha:")) for s in d), d
    q = __import__("predict").build_parser()
    for net in ("ema0", "ema1", "ema_both"):
        assert q.parse_args(["--ckpt", "x", "--net", net]).net == net


def _identity(alpha):
    from cmlpl_amd import HyperParams, NetShape
    from cmlpl_amd.checkpoint import make_identity
    return make_identity(NetShape(103, 11, 11, 103, 9), HyperParams(), 32, 32, 320, "0123456789abcdef", 6,
                         teacher_alpha=alpha)


def test_identity_gains_the_coefficient_only_with_a_teacher():
    from cmlpl_amd.checkpoint import check_identity
    off, on, other = _identity(None), _identity(0.95), _identity(0.9)
    assert sorted(off) == ["Q", "abi", "bt", "btu", "hp", "shape", "source_hash"]           # what it was
    assert on["teacher_alpha"] == 0.95 and {k: v for k, v in on.items() if k != "teacher_alpha"} == off
    check_identity(off, on)          # a state without a teacher loads into an engine with one
    check_identity(on, off)          # and the other way round (the engine leaves the teacher aside)
    check_identity(on, _identity(0.95))
    with pytest.raises(ValueError, match="teacher_alpha"):
        check_identity(on, other)


def test_ema_at_world_size_two_is_refused_before_any_device_call(monkeypatch):
    import train
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("LOCAL_RANK", "1")

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch.cuda, "set_device", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    args = train.build_parser().parse_args(["--ema", "--synthetic", "B2", "--no_eval"])
    with pytest.raises(SystemExit) as e:
        train.main(args)
    assert "--ema runs on one GPU" in str(e.value) and "\n" not in str(e.value)


def test_engine_refuses_a_coefficient_outside_the_unit_interval():
    from cmlpl_amd import NetShape
    from cmlpl_amd.engine import TrainEngine
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="teacher_alpha"):
            TrainEngine(NetShape(), 32, 32, teacher_alpha=bad)


def test_drop_in_is_exported_and_refuses_cpu_modules():
    import tools.models as tm
    from cmlpl_amd.models import WeightEMA_BN
    assert tm.WeightEMA_BN is WeightEMA_BN and "WeightEMA_BN" in tm.__all__
    _lib_loaded()
    a, b = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        WeightEMA_BN(a, b, 0.95)
    with pytest.raises(ValueError, match="alpha"):
        WeightEMA_BN(a, b, 1.5)
    with pytest.raises(ValueError, match="keys differ"):
        WeightEMA_BN(a, torch.nn.Sequential(torch.nn.Linear(3, 2)), 0.95)
