#!/usr/bin/env python3
"""What the EMA teacher costs, on one GPU, interleaved in one process:
    python scripts/bench_ema.py [--workloads B2,P] [--steps 100] [--windows 7] [--parent DIR] [--out FILE.json]
For each workload at 128 + 128 rows, by index over resident splits of --rows rows (seeded synthetic data):
  * the step with and without the teacher (TrainEngine(teacher_alpha=0.95) / None), eager and replayed from the captured
    graph: `--windows` timed windows of `--steps` steps per mode, the modes taken in turn inside every round (drift of the
    box hits all alike); median, min and max of the windows;
  * the update launch alone (cmlpl_ema_update over the engine's 2 x param_stride block) between event pairs: a burst of
    launches per pair, microseconds per launch;
  * one evaluation of the teacher (full pack of its weights + the list-fed forward + the confusion count) beside one of
    the student (forward + count: its packed weights ride with the step), on --eval-pixels pixels of a 64 x 64 scene; the
    teacher is marked changed in front of every timed evaluation, as a step would leave it.
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

SHAPES = {"B2": (103, 11, 11, 103, 9), "P": (60, 20, 20, 103, 9), "B5": (48, 15, 15, 48, 20)}
DEV = "cuda:0"
ALPHA = 0.95


def make_mode(shape, bt, btu, rows_split, teacher, graph, data):
    XP, X, Y, XPu, Xu, lp, up = data
    eng = TrainEngine(NetShape(*shape), bt, btu, HyperParams(), device=DEV, seed=1088, hist_rows=16,
                      teacher_alpha=ALPHA if teacher else None)
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


def update_alone(eng, pairs=20, burst=50):
    """microseconds per cmlpl_ema_update launch over the engine's block: `burst` launches between two events"""
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    scratch = eng.teacher_params.clone()            # (the teacher itself is left as the run made it)
    src, dst, n = eng.params.data_ptr(), scratch.data_ptr(), 2 * eng.P
    for _ in range(burst):
        _lib.check("cmlpl_ema_update", lib.cmlpl_ema_update(src, dst, n, ALPHA, st))
    us = []
    for _ in range(pairs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            _lib.check("cmlpl_ema_update", lib.cmlpl_ema_update(src, dst, n, ALPHA, st))
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) / burst * 1e3)
    return dict(spread(us), floats=n, bytes_moved=12 * n)


def evaluations(eng, shape, pixels, reps=15):
    """milliseconds per evaluation of the registered list: the student's, and the teacher's with its pack"""
    from cmlpl_amd.evaluate import Evaluator
    g = torch.Generator().manual_seed(3)
    Cc, _, _, bands, K = shape
    cube = torch.randn(64, 64, Cc, generator=g).to(DEV)
    X = torch.randn(64 * 64, bands, generator=g).to(DEV)
    pix = torch.randperm(64 * 64, generator=g)[:pixels].to(DEV)
    truth = torch.randint(0, K, (pixels,), generator=g).to(DEV)
    ev = Evaluator(NetShape(*shape), cube, X, truth, pix, spec_rows=pix)
    out = {}
    for name, nets in (("student", (eng, None)), ("teacher", (eng.teacher, None))):
        ms = []
        for i in range(reps + 2):
            if name == "teacher":
                eng.teacher._dirty = True           # as a step leaves it: the evaluation packs
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ev.evaluate(nets)
            b.record()
            b.synchronize()
            if i >= 2:
                ms.append(a.elapsed_time(b))
        out[name + "_ms"] = spread(ms)
    out["pixels"] = pixels
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
    ap.add_argument("--workloads", default="B2,P")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1024, help="rows per resident split")
    ap.add_argument("--eval-pixels", type=int, default=4096)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its own built library")
    ap.add_argument("--bench-reps", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"date": time.strftime("%Y-%m-%d"), "steps_per_window": args.steps, "windows": args.windows, "alpha": ALPHA,
           "workloads": {}}
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
        for teacher in (False, True):
            for gr in (False, True):
                modes[("ema" if teacher else "plain") + ("_graph" if gr else "_eager")] = make_mode(shape, bt, btu, n, teacher, gr, data)
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
        eng = modes["ema_eager"][0]
        out["update_us"] = update_alone(eng)
        from cmlpl_amd.infer import infer_fused
        if infer_fused(NetShape(*shape)):                       # (the list-fed fused forward; other windows go by patches)
            out["evaluation"] = evaluations(eng, shape, args.eval_pixels)
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
