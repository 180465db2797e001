"""CPU: the plumbing of the second training method (cross pseudo supervision) -- header / binding / exports, the
command lines, the checkpoint identity, the refusal of several GPUs.  No compute calls."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "cmlpl.h")).read()


def test_new_symbols_are_in_header_binding_and_library_together():
    from cmlpl_amd import _lib, build_ext
    if build_ext.needs_build():
        build_ext.build(verbose=False)
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("cmlpl_cps_loss_fwd_bwd", "cmlpl_cps_loss_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert len(lib.cmlpl_cps_loss_fwd_bwd.argtypes) == 12
    assert lib.cmlpl_abi_version() == 6                      # added after ABI 6, no bump
    m = re.search(r"CMLPL_METHOD_CMLPL\s*=\s*(\d+)\s*,\s*CMLPL_METHOD_CPS\s*=\s*(\d+)", code)
    assert m and _lib.METHODS == {"cmlpl": int(m.group(1)), "cps": int(m.group(2))} and _lib.METHODS["cmlpl"] == 0
    # the timing id of the new launch: the enum and the binding's names stay one list
    enum = re.search(r"enum\s*\{\s*CMLPL_K_AUGMENT.*?CMLPL_K_COUNT\s*\}", code, flags=re.S).group(0)
    ids = re.findall(r"CMLPL_K_[A-Z0-9_]+", enum)
    assert ids[-1] == "CMLPL_K_COUNT" and ids[-2] == "CMLPL_K_CPS_LOSS"
    assert len(ids) - 1 == len(_lib.KERNEL_NAMES) and _lib.KERNEL_NAMES[-1] == "cps_loss"
    sz = lib.cmlpl_cps_loss_workspace_bytes(C.byref(_lib.Shape(103, 11, 11, 103, 9)), 128, 128)
    assert sz >= 6 * 128 * 4 + 4
    assert lib.cmlpl_cps_loss_workspace_bytes(C.byref(_lib.Shape(103, 11, 11, 103, 65)), 128, 128) == 0


def test_no_record_changed_size():
    """the sizes ABI 6 callers were built against (sizeof of the records of the header before this method was added,
    x86-64 / LP64), in the binding"""
    from cmlpl_amd import _lib
    want = dict(Shape=20, HParams=48, Layout=288, Shard=24, Batch=104, Dyn=64, Banks=48, StepIO=296, Gathered=32)
    got = {k: C.sizeof(getattr(_lib, k)) for k in want}
    assert got == want, got
    assert _lib.StepIO.reserved.offset == _lib.StepIO.apply_update.offset + 4      # the method lives where `reserved` lay
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct cmlpl_step_io \{(.*?)\} cmlpl_step_io;", code, flags=re.S).group(1)
    assert re.search(r"int32_t apply_update;\s*int32_t reserved;", body)


def test_parser_defaults_to_cmlpl_and_takes_cps():
    import train
    p = train.build_parser()
    assert p.parse_args([]).method == "cmlpl"
    assert p.parse_args(["--method", "cps"]).method == "cps"
    with pytest.raises(SystemExit):
        p.parse_args(["--method", "cct"])


def test_trian_cps_help_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "trian_CPS.py"), "--help"], capture_output=True, text=True,
                       cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "--method" in r.stdout and "--labeled_batch_size" in r.stdout and "--noise" in r.stdout


def test_trian_cps_presets_the_method(monkeypatch):
    import runpy
    import train
    seen = {}
    monkeypatch.setattr(train, "main", lambda args: seen.update(method=args.method, bt=args.labeled_batch_size))
    monkeypatch.setattr(sys, "argv", ["trian_CPS.py", "--labeled_batch_size", "64"])
    runpy.run_path(os.path.join(ROOT, "trian_CPS.py"), run_name="__main__")
    assert seen == dict(method="cps", bt=64)


def _identity(method):
    from cmlpl_amd import HyperParams, NetShape
    from cmlpl_amd.checkpoint import make_identity
    return make_identity(NetShape(103, 11, 11, 103, 9), HyperParams(), 32, 32, 320, "0123456789abcdef", 6, method=method)


def test_checkpoint_identity_refuses_the_other_method_both_ways():
    from cmlpl_amd.checkpoint import check_identity
    a, b = _identity("cmlpl"), _identity("cps")
    check_identity(a, _identity("cmlpl"))
    check_identity(b, _identity("cps"))
    for saved, mine in ((a, b), (b, a)):
        with pytest.raises(ValueError) as e:
            check_identity(saved, mine)
        assert "'cmlpl'" in str(e.value) and "'cps'" in str(e.value) and "method" in str(e.value)


def test_a_cmlpl_identity_is_what_it_was_and_a_file_without_the_key_reads_as_cmlpl():
    from cmlpl_amd.checkpoint import check_identity, identity_method
    a = _identity("cmlpl")
    assert sorted(a) == ["Q", "abi", "bt", "btu", "hp", "shape", "source_hash"]          # no new key
    assert "method" in _identity("cps")
    assert identity_method(a) == "cmlpl" and identity_method(_identity("cps")) == "cps"
    parent = {k: v for k, v in a.items()}                     # a record written before there was a second method
    check_identity(parent, _identity("cmlpl"))
    with pytest.raises(ValueError, match="method"):
        check_identity(parent, _identity("cps"))


def test_a_cmlpl_run_record_is_what_it_was():
    import train
    from cmlpl_amd import HyperParams
    p = train.build_parser()
    a0, a1 = p.parse_args(["--synthetic", "B2"]), p.parse_args(["--synthetic", "B2", "--method", "cps"])
    r0 = train.run_record(a0, HyperParams(), train.SYNTH["B2"], False)
    r1 = train.run_record(a1, HyperParams(), train.SYNTH["B2"], False)
    assert "method" not in r0 and r1["method"] == "cps"
    assert {k: v for k, v in r1.items() if k != "method"} == r0


def test_unknown_method_is_refused_before_the_library_is_touched():
    from cmlpl_amd import NetShape
    from cmlpl_amd.engine import TrainEngine
    with pytest.raises(ValueError, match="cmlpl, cps"):
        TrainEngine(NetShape(), 32, 32, method="cct")


def test_cps_at_world_size_two_is_refused_before_any_device_call(monkeypatch):
    import train
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("LOCAL_RANK", "1")

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch.cuda, "set_device", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    args = train.build_parser().parse_args(["--method", "cps", "--synthetic", "B2", "--no_eval"])
    with pytest.raises(SystemExit) as e:
        train.main(args)
    assert "--method cps runs on one GPU" in str(e.value) and "\n" not in str(e.value)
    # the sharded engine itself: no CPS step, said before it looks for a device or a communicator
    from cmlpl_amd import NetShape
    from cmlpl_amd.distributed import DistTrainEngine
    with pytest.raises(ValueError, match="cps"):
        DistTrainEngine(NetShape(), 16, 16, method="cps")


def test_two_ranks_under_the_launcher_end_at_once_with_that_line():
    """as two real processes with the rendezvous variables set (cmlpl_amd.launch.spawn_ranks, as tests/test_dist_startup.py
    starts its ranks): both leave before any process group or device is touched"""
    from cmlpl_amd.launch import spawn_ranks
    t0 = time.monotonic()
    rc, _ = spawn_ranks(2, [sys.executable, os.path.join(ROOT, "train.py"), "--method", "cps", "--synthetic", "B2",
                            "--no_eval"], timeout=300, retries=0)
    assert rc != 0 and rc != 124
    assert time.monotonic() - t0 < 120
