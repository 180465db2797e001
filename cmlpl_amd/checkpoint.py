"""Checkpoints: the state a training run carries from one step to the next, as ONE file.

The reference keeps nothing (its train.py ends with the networks in device memory); this is the build's own.  What a
file holds is ``TrainEngine.checkpoint_state()`` -- the flat parameter / Adam buffers, both memory banks and their
pointers, the step counters that key the in-kernel noise and dropout streams, the two-piece range flag words of each
network, and an ``identity`` record that ``load_checkpoint_state`` checks (``check_identity``) -- plus ``"Base"`` and
``"Base1"``, the two networks as ``state_dict``s with the reference's 16 keys (they load into this package's
``BaseNet2`` and into the reference's class alike), plus -- from an engine that keeps an EMA teacher (``teacher_alpha``)
only -- ``teacher_params`` and ``"Teacher"`` / ``"Teacher1"``, the averaged weights in the same two forms, plus whatever the driver adds under ``"extra"`` (train.py: the
epoch reached, ``loss_hist`` so far, the validation curve, the permutation generator's state).

Tensors, numbers, strings, lists and dicts only: a file is read with ``torch.load(weights_only=True)``, nothing in it
is a pickled object.  ``save`` writes under a temporary name in the target's directory and renames: a run that is
killed while it writes leaves the previous file (or none) under the final name, never half a file.
"""
from __future__ import annotations

import os
import tempfile
import warnings
from typing import Any, Dict, List, Optional

import torch

FORMAT_VERSION = 1
STATE_TENSORS = ("params", "m", "v", "bank_feats", "bank_probs", "range_flags")
STATE_INTS = ("adam_t", "step_count", "seed")


class CheckpointError(RuntimeError):
    """a file that is not a checkpoint of this format"""


def make_identity(shape, hp, bt_global: int, btu_global: int, Q: int, source_hash: str, abi: int,
                  method: str = "cmlpl", teacher_alpha: Optional[float] = None, aug_spatial: str = "none",
                  optim=None) -> Dict[str, Any]:
    """the record ``check_identity`` compares: plain dicts and numbers (``NetShape`` / ``HyperParams`` by field).  The
    training ``method`` is part of it; a CMLPL record carries no ``method`` key (what it held before there was a second
    method: such files still load, and a record without the key reads as ``cmlpl``).  ``teacher_alpha``: the coefficient of
    an engine that keeps an EMA teacher -- a key only such an engine's record has (without one the record is what it was).
    ``aug_spatial``: the flip / rotate augmentation of the cube-fed step, a key only when it is not "none".
    ``optim`` (``cmlpl_amd.optim.OptimConfig``): ``weight_decay``, ``clip_grad`` and ``lr_schedule`` (the schedule's fields,
    ``total_steps`` among them), each a key only when it is not the default."""
    from dataclasses import asdict
    rec = dict(shape={k: int(v) for k, v in asdict(shape).items()},
               hp={k: (int(v) if isinstance(v, int) and not isinstance(v, bool) else float(v)) for k, v in asdict(hp).items()},
               bt=int(bt_global), btu=int(btu_global), Q=int(Q), source_hash=str(source_hash), abi=int(abi))
    if method != "cmlpl":
        rec["method"] = str(method)
    if teacher_alpha is not None:
        rec["teacher_alpha"] = float(teacher_alpha)
    if aug_spatial != "none":
        rec["aug_spatial"] = str(aug_spatial)
    if optim is not None:
        rec.update(optim.identity())
    return rec


def identity_method(rec: Dict[str, Any]) -> str:
    return str(rec.get("method", "cmlpl"))


def identity_differences(saved: Dict[str, Any], mine: Dict[str, Any]) -> List[str]:
    """every field of the two identity records that differs, as ``name: file X, here Y`` (``method``, ``shape.C``, ``hp.lr``,
    ``bt``, ``btu``, ``Q``, ``abi``); ``source_hash`` is not among them (another build of the same ABI computes the same step up
    to what its kernels changed: ``check_identity`` warns)."""
    out = []
    if identity_method(saved) != identity_method(mine):
        out.append(f"method: file {identity_method(saved)!r}, here {identity_method(mine)!r}")
    if saved.get("aug_spatial", "none") != mine.get("aug_spatial", "none"):
        out.append(f"aug_spatial: file {saved.get('aug_spatial', 'none')!r}, here {mine.get('aug_spatial', 'none')!r}")
    for group in ("shape", "hp"):
        a, b = saved.get(group, {}), mine.get(group, {})
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b or a[k] != b[k]:
                out.append(f"{group}.{k}: file {a.get(k, 'absent')!r}, here {b.get(k, 'absent')!r}")
    for k in ("bt", "btu", "Q", "abi"):
        if saved.get(k) != mine.get(k):
            out.append(f"{k}: file {saved.get(k)!r}, here {mine.get(k)!r}")
    # (a teacher on one side only is no difference: an engine with one starts it from the file's parameters, an engine
    #  without one leaves the file's aside -- two different coefficients are two different averages)
    if "teacher_alpha" in saved and "teacher_alpha" in mine and saved["teacher_alpha"] != mine["teacher_alpha"]:
        out.append(f"teacher_alpha: file {saved['teacher_alpha']!r}, here {mine['teacher_alpha']!r}")
    from .optim import optim_identity_differences
    out.extend(optim_identity_differences(saved, mine))
    return out


def check_identity(saved: Dict[str, Any], mine: Dict[str, Any]) -> None:
    """ValueError naming every differing field; a different ``source_hash`` alone is a warning"""
    diff = identity_differences(saved, mine)
    if diff:
        raise ValueError("the checkpoint was written by a different configuration -- " + "; ".join(diff))
    if saved.get("source_hash") != mine.get("source_hash"):
        warnings.warn(f"the checkpoint was written by another build of the kernels (source hash "
                      f"{saved.get('source_hash')}, this library {mine.get('source_hash')}): it loads, but a resumed run "
                      "need not continue bit for bit")


def _to_cpu(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _to_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_to_cpu(v) for v in x]
    return x


def save(path: str, state: Dict[str, Any], extra: Optional[Dict[str, Any]] = None) -> None:
    """Write ``state`` (``checkpoint_state()``; device tensors are copied to the host here -- one synchronisation) and
    the driver's ``extra`` as one file: under a temporary name beside ``path``, then ``os.replace``."""
    path = os.fspath(path)
    payload = {k: _to_cpu(v) for k, v in state.items()}
    payload["format_version"] = FORMAT_VERSION
    payload["extra"] = _to_cpu(dict(extra or {}))
    d = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=d)
    try:
        with os.fdopen(fd, "wb") as f:
            torch.save(payload, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def load(path: str, map_location="cpu") -> Dict[str, Any]:
    """the file as a dict (``weights_only=True``: tensors and plain values); CheckpointError for another format version"""
    ck = torch.load(os.fspath(path), map_location=map_location, weights_only=True)
    if not isinstance(ck, dict) or "format_version" not in ck:
        raise CheckpointError(f"{path}: not a cmlpl_amd checkpoint (no format_version)")
    if ck["format_version"] != FORMAT_VERSION:
        raise CheckpointError(f"{path}: checkpoint format version {ck['format_version']!r}, this build reads version "
                              f"{FORMAT_VERSION}")
    return ck


def load_networks(path: str, device="cuda:0"):
    """(Base, Base1) of a file as eval-mode ``cmlpl_amd.BaseNet2`` modules on ``device``"""
    from .models import BaseNet2
    ck = load(path)
    s, hp = ck["identity"]["shape"], ck["identity"]["hp"]
    if s["H"] != s["W"]:
        raise CheckpointError(f"{path}: BaseNet2 takes square windows, the file has {s['H']} x {s['W']}")
    nets = []
    for key in ("Base", "Base1"):
        m = BaseNet2(num_features=s["bands"], dropout=hp["dropout"], num_classes=s["K"], in_channels=s["C"],
                     window=s["H"]).to(device)
        m.load_state_dict(ck[key])
        nets.append(m.eval())
    return tuple(nets)
