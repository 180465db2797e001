#!/usr/bin/env python3
"""Split-fed step against cube-fed step (cmlpl_batch.d_cube, ABI 6) on one GPU, interleaved in one process:
    python scripts/bench_cube_feed.py [--workloads B2,P] [--steps 100] [--windows 7] [--out FILE.json]
For each workload at 128 + 128 rows, by index over resident splits of --rows rows cut from a seeded synthetic scene:
  * ms/step of the split-fed and the cube-fed step, eager and replayed from the captured graph -- `--windows` timed
    windows of `--steps` steps per mode, the modes taken in turn inside every round (so drift of the box hits all
    alike); median, min and max of the windows are reported (the spread IS the min / max);
  * the gather + augment launch alone (cmlpl_timing_begin/_end around CMLPL_K_CUBE_FEED) in microseconds;
  * resident bytes of the training data per mode (window tensors | cube + pixel lists; spectra / labels are common).
Run on a tree without the cube-fed step (the parent commit: the yardstick for the split-fed time) it reports the
split-fed modes only.  One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cmlpl_amd import HyperParams, NetShape, TrainEngine, _lib  # noqa: E402
from cmlpl_amd.patches import extract_patches  # noqa: E402

SHAPES = {"B2": (103, 11, 11, 103, 9), "P": (60, 20, 20, 103, 9), "B5": (48, 15, 15, 48, 20)}
DEV = "cuda:0"


def make_mode(shape, bt, btu, rows_split, cube_fed, graph, data):
    cube, lab_pix, unl_pix, X, Y, Xu, XP, XPu, lp, up = data
    eng = TrainEngine(NetShape(*shape), bt, btu, HyperParams(), device=DEV, seed=1088, hist_rows=16)
    eng.init_params_default(1088)
    src = dict(cube=cube, lab_pix=lab_pix, unl_pix=unl_pix) if cube_fed else {}
    a = (None, X, Y, None, Xu) if cube_fed else (XP, X, Y, XPu, Xu)
    nb = rows_split // max(bt, btu)
    state = {"k": 0}

    def eager():
        k = state["k"] % nb
        eng.step(*a, 1, 20 + k, lab_idx=lp[k * bt:(k + 1) * bt], unl_idx=up[k * btu:(k + 1) * btu], **src)
        state["k"] += 1
    eager()
    if not graph:
        return eng, lambda n: [eager() for _ in range(n)]
    g = eng.capture(*a, lp, up, bt, btu, capacity=4096, **src)

    def replay(n):
        g.program([(1, 20 + (state["k"] + i) % nb, ((state["k"] + i) % nb) * bt, ((state["k"] + i) % nb) * btu) for i in range(n)])
        for _ in range(n):
            g.launch()
        state["k"] += n
    return eng, replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="B2,P")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1024, help="rows per resident split")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    have_cube = getattr(TrainEngine, "takes_cube", False)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "cube_fed_step": bool(have_cube),
           "steps_per_window": args.steps, "windows": args.windows, "workloads": {}}
    bt = btu = 128
    for name in args.workloads.split(","):
        shape = SHAPES[name]
        Cc, H, W, bands, K = shape
        g = torch.Generator().manual_seed(7)
        rows, cols = 610, 340                                   # PaviaU's scene size
        cube = torch.randn(rows, cols, Cc, generator=g).to(DEV)
        n = args.rows
        lab_pix, unl_pix = (torch.randint(0, rows * cols, (n,), generator=g).to(DEV) for _ in range(2))
        X, Y, Xu = torch.randn(n, bands, generator=g).to(DEV), torch.randint(0, K, (n,), generator=g).to(DEV), torch.randn(n, bands, generator=g).to(DEV)
        XP, XPu = extract_patches(cube, lab_pix, H), extract_patches(cube, unl_pix, H)
        lp, up = torch.randperm(n, generator=g).to(DEV), torch.randperm(n, generator=g).to(DEV)
        data = (cube, lab_pix, unl_pix, X, Y, Xu, XP, XPu, lp, up)
        modes = {}
        for cf in ([False, True] if have_cube else [False]):
            for gr in (False, True):
                modes[("cube" if cf else "split") + ("_graph" if gr else "_eager")] = make_mode(shape, bt, btu, n, cf, gr, data)
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
        out = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in times.items()}
        if have_cube:
            nk = len(_lib.KERNEL_NAMES)
            kid = _lib.KERNEL_NAMES.index("cube_feed")
            ms, cnt = (C.c_double * nk)(), (C.c_int64 * nk)()
            lib = _lib.load()
            _lib.check("cmlpl_timing_begin", lib.cmlpl_timing_begin(1 << kid, 64))
            modes["cube_eager"][1](50)
            _lib.check("cmlpl_timing_end", lib.cmlpl_timing_end(ms, cnt))
            out["gather_kernel_us"] = ms[kid] / max(cnt[kid], 1) * 1e3
            out["gather_launches"] = int(cnt[kid])
            per = Cc * H * W * 4
            out["gather_bytes"] = {"read": (bt + btu) * per, "written": 2 * (bt + btu) * per}
            out["resident_bytes"] = {"split": XP.numel() * 4 + XPu.numel() * 4,
                                     "cube": cube.numel() * 4 + lab_pix.numel() * 8 + unl_pix.numel() * 8}
        res["workloads"][name] = out
        del modes, data, XP, XPu
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
