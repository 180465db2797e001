#!/usr/bin/env python3
"""What a learning-rate schedule, weight decay and gradient clipping cost, on one GPU, interleaved in one process:
    python scripts/bench_optim.py [--workloads B2,P] [--steps 100] [--windows 7] [--parent DIR] [--out FILE.json]
For each workload at 128 + 128 rows, by index over resident splits of --rows rows (seeded synthetic data):
  * the step with everything off (TrainEngine(optim=None)), with clipping alone (one grad-norm launch more, the Adam
    kernel's second instantiation) and with all three on (cosine schedule with warm-up, decay 0.05, clipping), eager and
    replayed from the captured graph: `--windows` timed windows of `--steps` steps per mode, the modes taken in turn
    inside every round (drift of the box hits all alike); median, min and max of the windows;
  * cmlpl_grad_norm alone (its two launches over the last step's gradients) between event pairs: a burst per pair,
    microseconds per call -- enqueued one by one (which the host's calls bound) and as one captured graph of the burst
    replayed (the launches back to back on the device).
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
from cmlpl_amd.optim import LRSchedule, OptimConfig  # noqa: E402

SHAPES = {"B2": (103, 11, 11, 103, 9), "P": (60, 20, 20, 103, 9)}
DEV = "cuda:0"
# clip_grad 0.5: under the norms these workloads have (every step clips, so the coefficient is not the constant 1)
CONFIGS = {"off": None, "clip": OptimConfig(clip_grad=0.5),
           "all": OptimConfig(schedule=LRSchedule("cosine", 5e-4, 10 ** 6, warmup_steps=100, lr_min=1e-5), weight_decay=0.05,
                              clip_grad=0.5)}


def make_mode(shape, bt, btu, rows_split, optim, graph, data):
    XP, X, Y, XPu, Xu, lp, up = data
    eng = TrainEngine(NetShape(*shape), bt, btu, HyperParams(), device=DEV, seed=1088, hist_rows=16, optim=optim)
    eng.init_params_default(1088)
    nb = rows_split // max(bt, btu)
    state = {"k": 0}

    def eager():
        k = state["k"] % nb
        eng.step(XP, X, Y, XPu, Xu, 1, 20 + k, lab_idx=lp[k * bt:(k + 1) * bt], unl_idx=up[k * btu:(k + 1) * btu])
        state["k"] += 1
    eager()
    if not graph:
        return eng, lambda n: [eager() for _ in range(n)]
    g = eng.capture(XP, X, Y, XPu, Xu, lp, up, bt, btu, capacity=4096)

    def replay(n):
        g.program([(1, 20 + (state["k"] + i) % nb, ((state["k"] + i) % nb) * bt, ((state["k"] + i) % nb) * btu) for i in range(n)])
        for _ in range(n):
            g.launch()
        state["k"] += n
    return eng, replay


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def launch_alone(eng, pairs=20, burst=50):
    """microseconds per cmlpl_grad_norm call (the partials launch and the fold) over the last step's gradients"""
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    norms = torch.zeros(4, device=eng.device)
    partials = torch.empty(lib.cmlpl_grad_norm_partials_bytes() // 8, dtype=torch.float64, device=eng.device)
    gp, pp, np_ = eng.grads.data_ptr(), partials.data_ptr(), norms.data_ptr()
    call = lambda: _lib.check("cmlpl_grad_norm", lib.cmlpl_grad_norm(C.byref(eng.cshape), 2, gp, eng.P, 0.5, pp, np_, st))
    for _ in range(burst):
        call()
    us = []
    for _ in range(pairs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            call()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) / burst * 1e3)
    # the same burst captured once and replayed: the eager loop above is bound by the host's calls (a ctypes call per
    # pair of launches), a replay runs the launches back to back on the device
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
        for _ in range(burst):
            call()
    st = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    graph.replay()
    replayed = []
    for _ in range(pairs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        replayed.append(a.elapsed_time(b) / burst * 1e3)
    live = int(sum(eng.layout.param_numel[:10]))
    return dict(spread(us), replayed=spread(replayed), launches_per_call=2, live_floats_per_net=live, norms=norms.tolist())


def bench_py(tree, steps, warmup):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed:\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="B2,P")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1024, help="rows per resident split")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its own built library")
    ap.add_argument("--bench-reps", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"date": time.strftime("%Y-%m-%d"), "steps_per_window": args.steps, "windows": args.windows, "workloads": {}}
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
    bt = btu = 128
    for name in args.workloads.split(","):
        shape = SHAPES[name]
        Cc, H, W, bands, K = shape
        g = torch.Generator().manual_seed(7)
        n = args.rows
        XP, XPu = (torch.randn(n, Cc, H, W, generator=g).to(DEV) for _ in range(2))
        X, Y, Xu = torch.randn(n, bands, generator=g).to(DEV), torch.randint(0, K, (n,), generator=g).to(DEV), torch.randn(n, bands, generator=g).to(DEV)
        lp, up = torch.randperm(n, generator=g).to(DEV), torch.randperm(n, generator=g).to(DEV)
        data = (XP, X, Y, XPu, Xu, lp, up)
        modes = {}
        for cname, cfg in CONFIGS.items():
            for gr in (False, True):
                modes[cname + ("_graph" if gr else "_eager")] = make_mode(shape, bt, btu, n, cfg, gr, data)
        times = {k: [] for k in modes}
        for k, (_, run) in modes.items():                      # warm every mode
            run(10)
        torch.cuda.synchronize()
        for _ in range(args.windows):
            for k, (_, run) in modes.items():                  # the modes in turn inside every round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(args.steps)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / args.steps * 1e3)
        out = {k: {"ms_" + kk: vv for kk, vv in spread(v).items()} for k, v in times.items()}
        eng = modes["all_eager"][0]
        out["last_norms_row"] = eng.grad_norms()
        out["grad_norm_us"] = launch_alone(eng)
        res["workloads"][name] = out
        del modes, data, XP, XPu, eng
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
