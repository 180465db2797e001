#!/usr/bin/env python3
"""What a checkpoint costs (docs/EXPERIMENTS.md "Checkpoints"): wall time of one epoch-end save (device -> host copy +
file write), of one --save_best device snapshot and of a load, on one GPU at the B2 defaults (128 + 128), host clock
around work that ends in a device synchronise, median of ``--reps`` repeats -- beside the wall time of an EPOCH, taken
from ``train.py``'s own "after the first epoch" line (eager and --graph) of the tree named by ``--epoch-tree`` (default:
this one; name a checkout of the parent commit to have its figure from the same call).  One JSON line."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def epoch_ms(tree, graph):
    """(ms per step after the first epoch, steps per epoch) of `train.py --synthetic B2 --num_epochs 4 --no_eval`"""
    cmd = [sys.executable, "train.py", "--synthetic", "B2", "--num_epochs", "4", "--no_eval"] + (["--graph"] if graph else [])
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    m = re.search(r"after the first epoch: (\d+) steps in ([\d.]+) s = ([\d.]+) ms/step", r.stdout)
    steps = int(m.group(1)) // 3
    return float(m.group(3)), steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--epoch-tree", default=ROOT)
    ap.add_argument("--no-epoch", action="store_true")
    a = ap.parse_args()
    import torch
    from cmlpl_amd import HyperParams, NetShape, TrainEngine, checkpoint
    from hsi_loader import SyntheticHSIDataSet
    shape = (103, 11, 11, 103, 9)
    dev = torch.device("cuda:0")
    eng = TrainEngine(NetShape(*shape), 128, 128, HyperParams(), device=dev, hist_rows=10)
    eng.init_params_default(1088)
    lab, unl = SyntheticHSIDataSet(shape, 512, 'label', seed=1), SyntheticHSIDataSet(shape, 512, 'unlabel', seed=2)
    (XPl, Xl, Y), (XPu, Xu, _) = lab.device_arrays(dev), unl.device_arrays(dev)
    idx = torch.arange(512, dtype=torch.int64, device=dev)
    for k in range(4):
        eng.step(XPl, Xl, Y, XPu, Xu, 0, k, lab_idx=idx[k * 128:(k + 1) * 128], unl_idx=idx[k * 128:(k + 1) * 128])
    torch.cuda.synchronize()
    extra = dict(epoch=1, loss_hist=torch.zeros(1560, 5, dtype=torch.float64), gen_state=torch.Generator().get_state())
    t = dict(state_to_host=[], file_write=[], save=[], snapshot=[], load_file=[], load_into_engine=[])
    snap = eng.checkpoint_state(on_device=True)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "bench.ckpt")
        for _ in range(a.reps + 1):                      # (the first repeat warms the allocator and the page cache)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = eng.checkpoint_state()
            t1 = time.perf_counter()
            checkpoint.save(path, st, extra)
            t2 = time.perf_counter()
            eng.checkpoint_state(on_device=True, into=snap)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            ck = checkpoint.load(path)
            t4 = time.perf_counter()
            eng.load_checkpoint_state(ck)
            torch.cuda.synchronize()
            t5 = time.perf_counter()
            for k, v in zip(t, (t1 - t0, t2 - t1, t2 - t0, t3 - t2, t4 - t3, t5 - t4)):
                t[k].append(v * 1e3)
        size = os.path.getsize(path)
    out = dict(device=torch.cuda.get_device_name(0), reps=a.reps, file_bytes=size,
               **{k + "_ms": round(statistics.median(v[1:]), 3) for k, v in t.items()},
               **{k + "_ms_min_max": [round(min(v[1:]), 3), round(max(v[1:]), 3)] for k, v in t.items()})
    if not a.no_epoch:
        for graph in (False, True):
            ms, steps = epoch_ms(a.epoch_tree, graph)
            out["epoch_%s_ms" % ("graph" if graph else "eager")] = round(ms * steps, 3)
            out["steps_per_epoch"] = steps
    print(json.dumps(out))


if __name__ == "__main__":
    main()
