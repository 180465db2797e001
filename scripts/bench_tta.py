#!/usr/bin/env python3
"""What test-time augmentation costs, on one GPU, in one process:
    python scripts/bench_tta.py [--scene 610x340] [--views 5] [--reps 9] [--parent DIR] [--out FILE.json]
B2 on a synthetic scene of --scene pixels (PaviaU's 610 x 340 by default), medians with min and max:
  * one noisy view (``infer_cube_view``: the view's spectra rows + the spectral branch + the fused forward that adds the
    noise while it stages its slab) against one clean ``infer_cube``, the two taken in turn; milliseconds per scene;
  * ``tta_cube`` of two networks x (1 + --views) views against ``ensemble_cube`` of the pair, in turn;
  * ``cmlpl_ensemble_views`` alone at 207,400 x 9 for 2 x (1 + --views) blocks against ``cmlpl_ensemble`` for 2, between
    event pairs: a burst of launches per pair, microseconds per launch; and ``cmlpl_ensemble_views`` at ONE view against
    ``cmlpl_ensemble`` for 2 and for 4 members, in turn.
`--parent DIR` (a checkout of the parent commit with its own built library): plain `bench.py --gpus 1` and
`scripts/bench_infer.py` there and here, in alternation, `--bench-reps` times each -- this tree's median must lie inside
the parent's own min .. max.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cmlpl_amd import HyperParams, NetShape, TrainEngine, _lib  # noqa: E402

B2 = (103, 11, 11, 103, 9)
DEV = "cuda:0"


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn, reps, warm=2):
    """milliseconds per call of fn between two events, after `warm` untimed calls"""
    ms = []
    for i in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return ms


def launches_alone(n, K, views, pairs=20, burst=50):
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    V = 1 + views
    z = (4 * torch.randn(2, V, n, K, generator=g)).to(DEV)
    labels = torch.empty(n, dtype=torch.int64, device=DEV)
    probs = torch.empty(n, K, device=DEV)
    conf, ent = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    dis = torch.empty(n, dtype=torch.int32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    out = (labels.data_ptr(), probs.data_ptr(), conf.data_ptr(), ent.data_ptr(), dis.data_ptr(), st)

    def views_burst():
        for _ in range(burst):
            _lib.check("cmlpl_ensemble_views", lib.cmlpl_ensemble_views(z.data_ptr(), 2, V, V * n * K, n * K, None, n, K, *out))

    def plain_burst():
        for _ in range(burst):
            _lib.check("cmlpl_ensemble", lib.cmlpl_ensemble(z.data_ptr(), 2, V * n * K, None, n, K, *out))
    res = {}
    for name, fn, blocks in (("ensemble_views", views_burst, 2 * V), ("ensemble", plain_burst, 2)):
        us = [t / burst * 1e3 for t in timed(fn, pairs)]
        moved = 4 * n * K * (blocks + 1) + n * (8 + 4 + 4 + 4)
        res[name + "_us"] = dict(spread(us), blocks=blocks, pixels=n, classes=K, bytes_moved=moved,
                                 gb_per_s_at_median=moved / (statistics.median(us) * 1e-6) / 1e9)
    # may the views kernel at ONE view stand in for cmlpl_ensemble?  The two in turn, for 2 and 4 members; its median must
    # lie inside cmlpl_ensemble's own min .. max
    z4 = (4 * torch.randn(4, n, K, generator=g)).to(DEV)
    for M in (2, 4):
        def plain_M():
            for _ in range(burst):
                _lib.check("cmlpl_ensemble", lib.cmlpl_ensemble(z4.data_ptr(), M, n * K, None, n, K, *out))

        def one_view_M():
            for _ in range(burst):
                _lib.check("cmlpl_ensemble_views", lib.cmlpl_ensemble_views(z4.data_ptr(), M, 1, n * K, n * K, None, n, K, *out))
        us = {"ensemble": [], "ensemble_views_one_view": []}
        plain_M(), one_view_M()
        for _ in range(pairs):
            for name, fn in (("ensemble", plain_M), ("ensemble_views_one_view", one_view_M)):
                us[name] += [t / burst * 1e3 for t in timed(fn, 1, warm=0)]
        r = {k: spread(v) for k, v in us.items()}
        r["inside_ensembles_spread"] = bool(r["ensemble"]["min"] <= r["ensemble_views_one_view"]["median"] <= r["ensemble"]["max"])
        res["one_view_%d_members_us" % M] = r
    return res


def scene(rows, cols, views, reps):
    from cmlpl_amd.ensemble import ensemble_cube
    from cmlpl_amd.infer import infer_cube
    from cmlpl_amd.tta import TTA, infer_cube_view, tta_cube
    eng = TrainEngine(NetShape(*B2), 32, 32, HyperParams(), device=DEV, seed=1088, hist_rows=8)
    eng.init_params_default(1088)
    g = torch.Generator().manual_seed(3)
    cube = torch.randn(rows, cols, B2[0], generator=g).to(DEV)
    X = torch.randn(rows * cols, B2[3], generator=g).to(DEV)
    tta = TTA(views, 0.5)
    modes = {"clean_infer_cube": lambda: infer_cube((eng, 0), cube, X, want_logits=True),
             "one_noisy_view": lambda: infer_cube_view((eng, 0), cube, X, tta, 0),
             "ensemble_cube_pair": lambda: ensemble_cube((eng, None), cube, X),
             "tta_cube_pair": lambda: tta_cube((eng, None), cube, X, tta)}
    times = {k: [] for k in modes}
    for fn in modes.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in modes.items():                              # the modes in turn inside every round
            times[k] += timed(fn, 1, warm=0)
    out = {k + "_ms": spread(v) for k, v in times.items()}
    out.update(scene=[rows, cols], views=views, blocks_per_network=1 + views)
    return out


def bench_py(tree, steps, warmup):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed:\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def bench_infer(tree):
    """scripts/bench_infer.py's B2 scene at 65,536 pixels per launch: its median, milliseconds"""
    r = subprocess.run([sys.executable, "scripts/bench_infer.py"], cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"scripts/bench_infer.py in {tree} failed:\n{r.stderr[-2000:]}")
    m = re.search(r"cube path,\s+65536 pixels per launch:\s+([0-9.]+) ms", r.stdout)
    return float(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=207400)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--scene", default="610x340")
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its own built library")
    ap.add_argument("--bench-reps", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"date": time.strftime("%Y-%m-%d")}
    if args.parent:
        # first, and in child processes only: this process has not touched the device yet
        parent = os.path.abspath(args.parent)
        for key, fn in (("bench_py_ms_per_step", lambda tree: bench_py(tree, args.bench_steps, args.bench_warmup)),
                        ("bench_infer_ms", bench_infer)):
            runs = {"parent": [], "this": []}
            for _ in range(args.bench_reps):
                runs["parent"].append(fn(parent))
                runs["this"].append(fn(ROOT))
            res[key] = {k: dict(spread(v), runs=v) for k, v in runs.items()}
            res[key]["inside_parents_spread"] = bool(res[key]["parent"]["min"] <= res[key]["this"]["median"] <= res[key]["parent"]["max"])
    res["device"] = torch.cuda.get_device_name(0)
    res["launch"] = launches_alone(args.pixels, args.classes, args.views)
    rows, cols = (int(v) for v in args.scene.split("x"))
    res["B2"] = scene(rows, cols, args.views, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
