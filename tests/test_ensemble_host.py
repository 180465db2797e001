"""CPU: the ensemble's plumbing -- the export, its binding and its argument checks (in front of any launch: no GPU), the
command lines, what a checkpoint keeps of them, and the fp64 statement of the definition that tests/test_gpu_ensemble.py
holds the kernel to (the reference has no ensemble: the definition is the yardstick)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer" (never dereferenced)


# ------------------------------------------------------------------ the definition, in numpy fp64
def first_max(p):
    """torch.max's index rule on the last axis: the first maximum; a NaN counts as the maximum, the first NaN wins"""
    nan = np.isnan(p)
    with np.errstate(invalid="ignore"):
        plain = np.argmax(np.where(nan, -np.inf, p), axis=-1)
    return np.where(nan.any(-1), np.argmax(nan, axis=-1), plain).astype(np.int64)


def top2_margin(p):
    """largest minus second largest along the last axis (inf for one class)"""
    if p.shape[-1] == 1:
        return np.full(p.shape[:-1], np.inf)
    s = np.sort(p, axis=-1)
    return s[..., -1] - s[..., -2]


def normalised_weights(weights, M):
    """w_m = weight_m / sum, formed in double and rounded to float -- what the kernel receives"""
    w = np.ones(M) if weights is None else np.asarray(weights, dtype=np.float64)
    return (w / w.sum()).astype(np.float32)


def ensemble_fp64(z, weights=None):
    """the definition on logits [M, n, K] (float32 values, fp64 arithmetic): dict of p_m [M, n, K], p [n, K], label [n],
    conf [n], entropy [n], disagree [n], label_m [M, n]"""
    z = np.asarray(z, dtype=np.float64)
    M = z.shape[0]
    w = normalised_weights(weights, M).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = np.exp(z - np.nanmax(np.where(np.isnan(z), -np.inf, z), axis=-1, keepdims=True))
        e = np.where(np.isnan(z).any(-1, keepdims=True), np.nan, e)
        pm = e / e.sum(-1, keepdims=True)
        p = np.zeros(z.shape[1:])
        for m in range(M):
            p = p + w[m] * pm[m]
        label = first_max(p)
        t = np.where(p == 0, 0.0, p * np.log(np.where(p == 0, 1.0, p)))
        label_m = first_max(pm)
    return dict(pm=pm, p=p, label=label, conf=np.take_along_axis(p, label[:, None], 1)[:, 0], entropy=-t.sum(-1),
                disagree=(label_m != label[None]).sum(0).astype(np.int32), label_m=label_m)


def ensemble_fp32_torch(z, weights=None):
    """the same in fp32 with torch on the CPU: its own error against fp64 is the yardstick of the device's"""
    zt = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))
    w = torch.from_numpy(normalised_weights(weights, zt.shape[0]))
    pm = torch.softmax(zt, -1)
    p = torch.zeros_like(pm[0])
    for m in range(zt.shape[0]):
        p = p + w[m] * pm[m]
    t = torch.where(p == 0, torch.zeros_like(p), p * torch.log(torch.where(p == 0, torch.ones_like(p), p)))
    return p.numpy(), (-t.sum(-1)).numpy()


def case_logits(K, M, n=4099):
    return (4.0 * np.random.default_rng(1000 * K + M).standard_normal((M, n, K))).astype(np.float32)


def test_fp64_definition_agrees_with_torch_on_a_small_case():
    z = case_logits(9, 2, n=257)
    want = torch.softmax(torch.from_numpy(z).double(), -1).mean(0)
    got = ensemble_fp64(z)
    assert np.abs(got["p"] - want.numpy()).max() < 1e-15
    assert np.array_equal(got["label"], want.argmax(1).numpy())
    assert np.abs(got["conf"] - want.max(1)[0].numpy()).max() < 1e-15
    ent = -(want * want.log()).sum(1).numpy()
    assert np.abs(got["entropy"] - ent).max() < 1e-13
    assert np.abs(got["p"].sum(1) - 1).max() < 1e-14 and got["disagree"].max() <= 2
    # the rules the kernel is held to, on rows made for them
    z2 = z[:, :4].copy()
    z2[0, 0, 3] = np.nan                       # a NaN in one member: the whole row is NaN, the label is the first NaN
    z2[:, 1, :] = -np.inf; z2[:, 1, 5] = 0.0   # -inf everywhere but one class
    z2[:, 2, 2] = z2[:, 2, 6] = 50.0           # two equal tops in every member: the lower index
    g = ensemble_fp64(z2)
    assert g["label"][0] == 0 and np.isnan(g["p"][0]).all() and np.isnan(g["conf"][0]) and np.isnan(g["entropy"][0])
    assert g["label"][1] == 5 and g["conf"][1] == 1.0 and g["entropy"][1] == 0.0 and (np.delete(g["p"][1], 5) == 0).all()
    assert g["label"][2] == 2 and g["p"][2, 2] == g["p"][2, 6]
    t = torch.from_numpy(z2[0, :1])
    assert int(torch.max(torch.softmax(t, -1), 1)[1]) == 0 and torch.isnan(torch.softmax(t, -1)).all()      # torch's rule


def test_the_fp32_yardstick_and_the_margins_of_the_gpu_cases():
    """what tests/test_gpu_ensemble.py relies on: the fp32 restatement's own error is a few 1e-7, and the label margin
    leaves out well under 1 % of a case"""
    for K, M in ((2, 2), (9, 2), (64, 4)):
        z = case_logits(K, M)
        ref = ensemble_fp64(z)
        p32, e32 = ensemble_fp32_torch(z)
        ep, ee = np.abs(p32 - ref["p"]).max(), np.abs(e32 - ref["entropy"]).max()
        out = float((top2_margin(ref["p"]) < 1e-5).mean())
        print("K %d M %d: fp32 torch-CPU error p %.2e entropy %.2e, pixels under the margin %.4f" % (K, M, ep, ee, out))
        assert 0 < ep < 1e-6 and 0 < ee < 2e-6 and out <= 0.002


# ------------------------------------------------------------------ the export
def _lib_loaded():
    from cmlpl_amd import _lib, build_ext
    if build_ext.needs_build():
        build_ext.build(verbose=False)
    return _lib, _lib.load()


def test_export_header_binding_and_version():
    _lib, lib = _lib_loaded()
    assert "cmlpl_ensemble" in _lib.EXPORTS and hasattr(lib, "cmlpl_ensemble")
    assert _lib.ABI_VERSION == 6 and lib.cmlpl_abi_version() == 6           # added after ABI 6, no bump
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cmlpl.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+cmlpl_ensemble\s*\(([^)]*)\)\s*;", code)
    assert m
    params = [" ".join(p.split()[:-1]) + "*" * p.split()[-1].count("*") for p in m.group(1).split(",")]
    assert params == ["const float*", "int", "int64_t", "const float*", "int", "int", "int64_t*", "float*", "float*",
                      "float*", "int32_t*", "void*"], params
    vp = C.c_void_p
    assert list(lib.cmlpl_ensemble.argtypes) == [vp, C.c_int, C.c_int64, C.POINTER(C.c_float), C.c_int, C.c_int,
                                                 vp, vp, vp, vp, vp, vp]
    assert lib.cmlpl_ensemble.restype is C.c_int
    from cmlpl_amd import build_ext
    assert "ensemble.hip" in build_ext.SOURCES
    assert C.sizeof(_lib.StepIO) == 296 and C.sizeof(_lib.Dyn) == 64        # no record changed size
    import cmlpl_amd
    from cmlpl_amd import ensemble
    for name in ("ensemble_logits", "ensemble_cube", "ensemble_pixels"):
        assert getattr(cmlpl_amd, name) is getattr(ensemble, name)


def _call(lib, members=2, stride=None, weights=None, n=16, K=9, logits=FAKE, labels=FAKE):
    w = None if weights is None else (C.c_float * len(weights))(*weights)
    return lib.cmlpl_ensemble(logits, members, n * K if stride is None else stride, w, n, K, labels, None, None, None,
                              None, None)


def test_argument_checks_return_e_arg_before_any_launch():
    """every call here is refused on the host: had one of them launched, it would have failed another way on this
    machine, which has no device"""
    _, lib = _lib_loaded()
    for members in (0, 5, -1):
        assert _call(lib, members=members) == E_ARG, members
    for K in (0, 65, -3):
        assert _call(lib, K=K) == E_ARG, K
    for n in (0, -1):
        assert _call(lib, n=n) == E_ARG, n
    nan, inf = float("nan"), float("inf")
    for w in ((-1.0, 2.0), (nan, 1.0), (1.0, nan), (0.0, 0.0), (inf, 1.0), (1.0, -0.5)):
        assert _call(lib, weights=w) == E_ARG, w
    assert _call(lib, members=1, weights=(0.0,)) == E_ARG
    assert _call(lib, logits=None) == E_ARG and _call(lib, labels=None) == E_ARG
    assert _call(lib, stride=16 * 9 - 1) == E_ARG                # the members' blocks would overlap
    assert _call(lib, logits=FAKE + 2) == E_ARG and _call(lib, labels=FAKE + 4) == E_ARG
    assert lib.cmlpl_ensemble(FAKE, 2, 144, None, 16, 9, FAKE, FAKE + 1, None, None, None, None) == E_ARG


def test_host_wrappers_refuse_what_they_cannot_take():
    from cmlpl_amd.ensemble import _groups, _weights, ensemble_logits
    with pytest.raises(ValueError, match="cuda"):
        ensemble_logits(torch.zeros(2, 4, 9))
    with pytest.raises(ValueError, match="weights"):
        _weights((1.0, 2.0, 3.0), 2)
    assert _weights(None, 2) is None and list(_weights((3, 1), 2)) == [3.0, 1.0]
    mods = [torch.nn.Linear(2, 2) for _ in range(5)]
    assert _groups(mods[:4])[1] == 4 and _groups(tuple(mods[:2]))[1] == 2 and _groups(mods[0])[1] == 1
    with pytest.raises(ValueError, match="members"):
        _groups(mods)
    with pytest.raises(ValueError, match="members"):
        _groups([])


# ------------------------------------------------------------------ the command lines
def test_parsers_take_the_new_flags():
    import predict
    import train
    p = train.build_parser()
    assert p.parse_args(["--synthetic", "B2"]).ensemble is False
    assert p.parse_args(["--synthetic", "B2", "--ensemble"]).ensemble is True
    assert train.NET_TAGS["ens"] == "_ens"
    q = predict.build_parser()
    for net in ("ensemble", "ensemble_all"):
        a = q.parse_args(["--ckpt", "x", "--net", net, "--proba", "p.npy", "--confidence", "c.npy", "--entropy", "e.npy"])
        assert (a.net, a.proba, a.confidence, a.entropy) == (net, "p.npy", "c.npy", "e.npy")
        predict.check_args(a)
    a = q.parse_args(["--ckpt", "x"])
    assert a.proba is None and a.confidence is None and a.entropy is None
    predict.check_args(q.parse_args(["--ckpt", "x", "--net", "ema1", "--entropy", "e.npy"]))
    for net in ("both", "ema_both"):
        for flag in ("--proba", "--confidence", "--entropy"):
            with pytest.raises(SystemExit) as e:
                predict.check_args(q.parse_args(["--ckpt", "x", "--net", net, flag, "f.npy"]))
            assert "--net " + net in str(e.value)
        predict.check_args(q.parse_args(["--ckpt", "x", "--net", net]))


def test_proba_with_both_exits_before_any_device_call(monkeypatch):
    import predict

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch.cuda, "set_device", boom)
    with pytest.raises(SystemExit):
        predict.main(predict.build_parser().parse_args(["--ckpt", "nowhere.pt", "--net", "both", "--proba", "p.npy"]))


def test_saved_args_and_run_record_without_the_flag_are_what_they_were():
    import train
    from cmlpl_amd import HyperParams
    from tests.test_gpu_ema import PARENT_ARGS, PARENT_RUN
    p = train.build_parser()
    a0 = p.parse_args(["--synthetic", "B2"])
    a1 = p.parse_args(["--synthetic", "B2", "--ensemble"])
    s0, s1 = train.saved_args(a0), train.saved_args(a1)
    assert "ensemble" not in s0 and set(s0) == PARENT_ARGS
    assert s1["ensemble"] is True and {k: v for k, v in s1.items() if k != "ensemble"} == s0
    assert set(train.saved_args(p.parse_args(["--synthetic", "B2", "--ema", "--method", "cps"]))) == \
        PARENT_ARGS | {"ema", "method"}
    # the ensemble is a way of LOOKING at a run: two legs of one run may differ in it
    r0, r1 = (train.run_record(a, HyperParams(), train.SYNTH["B2"], False) for a in (a0, a1))
    assert r0 == r1 and set(r0) == PARENT_RUN and train.run_differences(r0, r1) == []
