#!/usr/bin/env python3
"""What the spatial smoothing of the class probability maps costs, on one GPU, in one process:
    python scripts/bench_smooth.py [--scene 610x340] [--classes 9] [--channels 60] [--parent DIR] [--out FILE.json]
  * the launch alone (cmlpl_smooth_probs with every output) on a --scene x --classes map under a --channels cube, for
    R in 1, 2, 4, 8 and G in 0, 3, between event pairs: a burst of launches per pair, microseconds per launch (medians);
  * the same definition written in plain torch on the device (shifted slices of padded tensors, one tap at a time) --
    what a user would have written without the kernel -- between event pairs, milliseconds;
  * the bytes-once floor of the launch: rows * cols * (2 K + G) * 4 bytes at the HBM rate a float4 copy measures on an
    MI355X (6.29 TB/s);
  * ``smooth_cube`` of the two networks of a B2 engine against ``ensemble_cube`` of the same pair on a synthetic scene
    of --scene pixels, the two taken in turn; milliseconds per scene.
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
HBM_BYTES_PER_S = 6.29e12      # a float4 copy on an MI355X (8.0 TB/s is the specification)


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


def torch_smooth(p, cube, R, sigma_s, sigma_r, G):
    """the definition in plain torch: q [rows * cols, K] and its labels; taps outside the scene get weight 0"""
    rows, cols, _ = cube.shape
    K = p.shape[1]
    a, b = 1.0 / (2.0 * sigma_s * sigma_s), 1.0 / (2.0 * sigma_r * sigma_r)
    P = torch.nn.functional.pad(p.view(rows, cols, K), (0, 0, R, R, R, R))
    g = torch.nn.functional.pad(cube[:, :, :G], (0, 0, R, R, R, R))
    inside = torch.nn.functional.pad(torch.ones(rows, cols, device=p.device), (R, R, R, R))
    num, den = torch.zeros(rows, cols, K, device=p.device), torch.zeros(rows, cols, device=p.device)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            ys, xs = slice(R + dy, R + dy + rows), slice(R + dx, R + dx + cols)
            e = torch.full((rows, cols), (dy * dy + dx * dx) * a, device=p.device)
            if G:
                e = e + b * ((cube[:, :, :G] - g[ys, xs]) ** 2).sum(2)
            w = torch.exp(-e) * inside[ys, xs]
            num += w.unsqueeze(2) * P[ys, xs]
            den += w
    q = (num / den.unsqueeze(2)).view(rows * cols, K)
    return q, q.argmax(1)


def launch_and_torch(rows, cols, K, channels, pairs=15, burst=20):
    lib = _lib.load()
    gen = torch.Generator().manual_seed(5)
    n = rows * cols
    p = torch.softmax(2 * torch.randn(n, K, generator=gen), 1).to(DEV)
    cube = torch.randn(rows, cols, channels, generator=gen).to(DEV)
    out = torch.empty(n, K, device=DEV)
    labels = torch.empty(n, dtype=torch.int64, device=DEV)
    conf, ent = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    res = []
    for R in (1, 2, 4, 8):
        for G in (0, 3):
            ss, sr = R / 2.0, 0.5

            def burst_of_launches():
                for _ in range(burst):
                    _lib.check("cmlpl_smooth_probs", lib.cmlpl_smooth_probs(
                        p.data_ptr(), cube.data_ptr() if G else None, channels, G, rows, cols, K, R, ss, sr, out.data_ptr(),
                        labels.data_ptr(), conf.data_ptr(), ent.data_ptr(), st))
            us = [t / burst * 1e3 for t in timed(burst_of_launches, pairs)]
            q, lab = torch_smooth(p, cube, R, ss, sr, G)
            err = float((q - out).abs().max())
            t_ms = timed(lambda: torch_smooth(p, cube, R, ss, sr, G), 5, warm=1)
            floor = n * (2 * K + G) * 4
            res.append(dict(R=R, G=G, launch_us=spread(us), torch_ms=spread(t_ms), max_abs_difference_from_torch=err,
                            labels_equal_torch=float((lab == labels).float().mean()), floor_bytes=floor,
                            floor_us=floor / HBM_BYTES_PER_S * 1e6,
                            torch_over_launch=statistics.median(t_ms) * 1e3 / statistics.median(us)))
    return dict(scene=[rows, cols], classes=K, channels=channels, cases=res)


def scene(rows, cols, reps):
    from cmlpl_amd.ensemble import ensemble_cube
    from cmlpl_amd.infer import infer_cube
    from cmlpl_amd.smooth import Smooth, smooth_cube
    eng = TrainEngine(NetShape(*B2), 32, 32, HyperParams(), device=DEV, seed=1088, hist_rows=8)
    eng.init_params_default(1088)
    g = torch.Generator().manual_seed(3)
    cube = torch.randn(rows, cols, B2[0], generator=g).to(DEV)
    X = torch.randn(rows * cols, B2[3], generator=g).to(DEV)
    modes = {"infer_cube": lambda: infer_cube((eng, 0), cube, X),
             "ensemble_cube_probs": lambda: ensemble_cube((eng, None), cube, X, probs=True),
             "smooth_cube_R2": lambda: smooth_cube((eng, None), cube, X, Smooth(2), probs=True),
             "smooth_cube_R4": lambda: smooth_cube((eng, None), cube, X, Smooth(4), probs=True),
             "smooth_cube_R4_2_passes": lambda: smooth_cube((eng, None), cube, X, Smooth(4, iters=2), probs=True)}
    times = {k: [] for k in modes}
    for fn in modes.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in modes.items():                              # the modes in turn inside every round
            times[k] += timed(fn, 1, warm=0)
    out = {k + "_ms": spread(v) for k, v in times.items()}
    out.update(scene=[rows, cols])
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
    ap.add_argument("--scene", default="610x340")
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--channels", type=int, default=60)
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
    rows, cols = (int(v) for v in args.scene.split("x"))
    res["launch"] = launch_and_torch(rows, cols, args.classes, args.channels)
    res["B2"] = scene(rows, cols, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
