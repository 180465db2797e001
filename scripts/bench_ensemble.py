#!/usr/bin/env python3
"""What the ensemble costs, on one GPU, in one process:
    python scripts/bench_ensemble.py [--pixels 207400] [--classes 9] [--scene 610x340] [--parent DIR] [--out FILE.json]
  * the launch alone (cmlpl_ensemble with every output) on --pixels x --classes logits of 2 and of 4 members, between
    event pairs: a burst of launches per pair, microseconds per launch, and the bytes it moves over that time;
  * ``ensemble_cube`` of the two networks of a B2 engine against two plain ``infer_cube`` calls on a synthetic scene of
    --scene pixels (PaviaU's 610 x 340 by default), the two taken in turn; milliseconds per scene;
  * ``Evaluator.evaluate`` with and without ``ensemble`` on --eval-pixels pixels of that scene, in turn.
`--parent DIR` (a checkout of the parent commit with its own built library): plain `bench.py --gpus 1` there and here,
in alternation, `--bench-reps` times each -- the default path must lie inside the parent's own spread.  One JSON line."""
import argparse
import ctypes as C
import json
import os
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


def launch_alone(n, K, M, pairs=20, burst=50):
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    z = (4 * torch.randn(M, n, K, generator=g)).to(DEV)
    labels = torch.empty(n, dtype=torch.int64, device=DEV)
    probs = torch.empty(n, K, device=DEV)
    conf, ent = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    dis = torch.empty(n, dtype=torch.int32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def burst_of_launches():
        for _ in range(burst):
            _lib.check("cmlpl_ensemble", lib.cmlpl_ensemble(z.data_ptr(), M, n * K, None, n, K, labels.data_ptr(),
                                                            probs.data_ptr(), conf.data_ptr(), ent.data_ptr(),
                                                            dis.data_ptr(), st))
    us = [t / burst * 1e3 for t in timed(burst_of_launches, pairs)]
    moved = 4 * n * K * (M + 1) + n * (8 + 4 + 4 + 4)
    return dict(spread(us), members=M, pixels=n, classes=K, bytes_moved=moved,
                gb_per_s_at_median=moved / (statistics.median(us) * 1e-6) / 1e9)


def scene_and_evaluation(rows, cols, eval_pixels, reps):
    from cmlpl_amd.ensemble import ensemble_cube
    from cmlpl_amd.evaluate import Evaluator
    from cmlpl_amd.infer import infer_cube
    eng = TrainEngine(NetShape(*B2), 32, 32, HyperParams(), device=DEV, seed=1088, hist_rows=8)
    eng.init_params_default(1088)
    g = torch.Generator().manual_seed(3)
    cube = torch.randn(rows, cols, B2[0], generator=g).to(DEV)
    X = torch.randn(rows * cols, B2[3], generator=g).to(DEV)
    modes = {"two_infer_cube": lambda: (infer_cube((eng, 0), cube, X), infer_cube((eng, 1), cube, X)),
             "ensemble_cube": lambda: ensemble_cube((eng, None), cube, X),
             "ensemble_cube_all_outputs": lambda: ensemble_cube((eng, None), cube, X, probs=True, conf=True, entropy=True,
                                                                disagree=True)}
    pix = torch.randperm(rows * cols, generator=g)[:eval_pixels].to(DEV)
    truth = torch.randint(0, B2[4], (eval_pixels,), generator=g).to(DEV)
    ev = Evaluator(NetShape(*B2), cube, X, truth, pix, spec_rows=pix)
    modes["evaluate"] = lambda: ev.evaluate((eng, None))
    modes["evaluate_ensemble"] = lambda: ev.evaluate((eng, None), ensemble=True)
    times = {k: [] for k in modes}
    for fn in modes.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in modes.items():                              # the modes in turn inside every round
            times[k] += timed(fn, 1, warm=0)
    out = {k + "_ms": spread(v) for k, v in times.items()}
    out.update(scene=[rows, cols], eval_pixels=eval_pixels)
    return out


def bench_py(tree, steps, warmup):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed:\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=207400)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--scene", default="610x340")
    ap.add_argument("--eval-pixels", type=int, default=42776)
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
        runs = {"parent": [], "this": []}
        for _ in range(args.bench_reps):
            runs["parent"].append(bench_py(os.path.abspath(args.parent), args.bench_steps, args.bench_warmup))
            runs["this"].append(bench_py(ROOT, args.bench_steps, args.bench_warmup))
        res["bench_py_ms_per_step"] = {k: dict(spread(v), runs=v) for k, v in runs.items()}
        p, t = res["bench_py_ms_per_step"]["parent"], res["bench_py_ms_per_step"]["this"]
        res["bench_py_inside_parents_spread"] = bool(p["min"] <= t["median"] <= p["max"])
    res["device"] = torch.cuda.get_device_name(0)
    res["launch_us"] = [launch_alone(args.pixels, args.classes, M) for M in (2, 4)]
    rows, cols = (int(v) for v in args.scene.split("x"))
    res["B2"] = scene_and_evaluation(rows, cols, args.eval_pixels, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
