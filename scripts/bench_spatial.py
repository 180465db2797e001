#!/usr/bin/env python3
"""What flip / rotate windows cost, on one GPU:
    python scripts/bench_spatial.py [--steps 100] [--windows 7] [--parent DIR] [--out FILE.json]
Medians with min and max, the things compared taken in turn:
  (a) the gather + augment launch alone (cmlpl_timing_begin/_end around CMLPL_K_CUBE_FEED) at B2 and P, 128 + 128 rows, for
      aug_spatial none / flips / d4: microseconds per launch;
  (b) the cube-fed step, eager and replayed from its graph, none against d4: milliseconds per step;
  (c) `--parent DIR` (a checkout of the parent commit with its own built library): scripts/bench_tta.py there and here in
      alternation -- one noisy fused view and tta_cube of 2 networks x (1 + 5) views, at the identity: the TTA kernels
      execute the remap even then, the one non-default path that changed;
  (d) `--parent DIR`: plain `bench.py --gpus 1` and scripts/bench_infer.py there and here in alternation, `--bench-reps`
      times each.
For (c) and (d) this tree's median must lie inside the parent's own min .. max.  One JSON line."""
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

SHAPES = {"B2": (103, 11, 11, 103, 9), "P": (60, 20, 20, 103, 9)}
DEV = "cuda:0"


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def make_mode(shape, bt, btu, n, mode, graph, data):
    cube, lab_pix, unl_pix, X, Y, Xu, lp, up = data
    eng = TrainEngine(NetShape(*shape), bt, btu, HyperParams(), device=DEV, seed=1088, hist_rows=16, aug_spatial=mode)
    eng.init_params_default(1088)
    src = dict(cube=cube, lab_pix=lab_pix, unl_pix=unl_pix)
    nb = n // max(bt, btu)
    state = {"k": 0}

    def eager():
        k = state["k"] % nb
        eng.step(None, X, Y, None, Xu, 1, 20 + k, lab_idx=lp[k * bt:(k + 1) * bt], unl_idx=up[k * btu:(k + 1) * btu], **src)
        state["k"] += 1
    eager()
    if not graph:
        return lambda steps: [eager() for _ in range(steps)]
    g = eng.capture(None, X, Y, None, Xu, lp, up, bt, btu, capacity=4096, **src)

    def replay(steps):
        g.program([(1, 20 + (state["k"] + i) % nb, ((state["k"] + i) % nb) * bt, ((state["k"] + i) % nb) * btu) for i in range(steps)])
        for _ in range(steps):
            g.launch()
        state["k"] += steps
    return replay


def steps_and_gather(name, steps, windows, rows_split=1024):
    shape = SHAPES[name]
    Cc, H, W, bands, K = shape
    bt = btu = 128
    g = torch.Generator().manual_seed(7)
    rows, cols = 610, 340                                   # PaviaU's scene size
    cube = torch.randn(rows, cols, Cc, generator=g).to(DEV)
    n = rows_split
    lab_pix, unl_pix = (torch.randint(0, rows * cols, (n,), generator=g).to(DEV) for _ in range(2))
    X, Y, Xu = torch.randn(n, bands, generator=g).to(DEV), torch.randint(0, K, (n,), generator=g).to(DEV), torch.randn(n, bands, generator=g).to(DEV)
    lp, up = torch.randperm(n, generator=g).to(DEV), torch.randperm(n, generator=g).to(DEV)
    data = (cube, lab_pix, unl_pix, X, Y, Xu, lp, up)
    modes = {"%s_%s" % (m, "graph" if gr else "eager"): make_mode(shape, bt, btu, n, m, gr, data)
             for m in ("none", "d4") for gr in (False, True)}
    times = {k: [] for k in modes}
    for run in modes.values():
        run(10)
    torch.cuda.synchronize()
    for _ in range(windows):
        for k, run in modes.items():                        # the modes in turn inside every round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(steps)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / steps * 1e3)
    out = {"step_ms": {k: spread(v) for k, v in times.items()}}
    # the gather launch alone: event pairs around it inside eager steps, the three modes in turn
    eager = {m: (modes[m + "_eager"] if m != "flips" else make_mode(shape, bt, btu, n, m, False, data)) for m in ("none", "flips", "d4")}
    nk, kid = len(_lib.KERNEL_NAMES), _lib.KERNEL_NAMES.index("cube_feed")
    lib = _lib.load()
    us = {m: [] for m in eager}
    for _ in range(windows):
        for m, run in eager.items():
            ms, cnt = (C.c_double * nk)(), (C.c_int64 * nk)()
            _lib.check("cmlpl_timing_begin", lib.cmlpl_timing_begin(1 << kid, 64))
            run(50)
            _lib.check("cmlpl_timing_end", lib.cmlpl_timing_end(ms, cnt))
            us[m].append(ms[kid] / max(cnt[kid], 1) * 1e3)
    per = Cc * H * W * 4
    out["gather_us"] = {m: spread(v) for m, v in us.items()}
    out["gather_bytes"] = {"read": (bt + btu) * per, "written": 2 * (bt + btu) * per}
    return out


def child_json(tree, *cmd):
    r = subprocess.run([sys.executable, *cmd], cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} in {tree} failed:\n{r.stderr[-2000:]}")
    return r.stdout


def bench_py(tree, steps, warmup):
    out = child_json(tree, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup))
    return float(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["ms_per_step"])


def bench_infer(tree):
    m = re.search(r"cube path,\s+65536 pixels per launch:\s+([0-9.]+) ms", child_json(tree, "scripts/bench_infer.py"))
    return float(m.group(1))


def bench_tta(tree):
    """scripts/bench_tta.py's B2 scene: the medians of one noisy view and of tta_cube, 2 networks x (1 + 5) views, ms"""
    d = json.loads([ln for ln in child_json(tree, "scripts/bench_tta.py").splitlines() if ln.startswith("{")][-1])["B2"]
    return d["one_noisy_view_ms"]["median"], d["tta_cube_pair_ms"]["median"]


def against_parent(parent, args):
    res = {}
    alternations = [("bench_py_ms_per_step", lambda tree: bench_py(tree, args.bench_steps, args.bench_warmup), args.bench_reps),
                    ("bench_infer_ms", bench_infer, args.bench_reps), ("bench_tta", bench_tta, args.tta_reps)]
    for key, fn, reps in alternations:
        runs = {"parent": [], "this": []}
        for _ in range(reps):
            runs["parent"].append(fn(parent))
            runs["this"].append(fn(ROOT))
        if key == "bench_tta":
            for i, sub in enumerate(("one_noisy_view_ms", "tta_cube_pair_ms")):
                res[sub] = {k: dict(spread([r[i] for r in v]), runs=[r[i] for r in v]) for k, v in runs.items()}
        else:
            res[key] = {k: dict(spread(v), runs=v) for k, v in runs.items()}
    for v in res.values():
        v["inside_parents_spread"] = bool(v["parent"]["min"] <= v["this"]["median"] <= v["parent"]["max"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="B2,P")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its own built library")
    ap.add_argument("--bench-reps", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--tta-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"date": time.strftime("%Y-%m-%d")}
    if args.parent:      # first, and in child processes only: this process has not touched the device yet
        res["against_parent"] = against_parent(os.path.abspath(args.parent), args)
    res["device"] = torch.cuda.get_device_name(0)
    res["steps_per_window"], res["windows"] = args.steps, args.windows
    res["workloads"] = {}
    for name in args.workloads.split(","):
        res["workloads"][name] = steps_and_gather(name, args.steps, args.windows)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
