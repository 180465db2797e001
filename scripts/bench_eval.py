#!/usr/bin/env python3
"""What validation costs, on one GPU, the modes interleaved in one process:
    python scripts/bench_eval.py [--workloads B2] [--reps 5] [--windows 7] [--out FILE.json]
A PaviaU-sized synthetic scene (610 x 340) and a seeded list of 42,776 distinct "test" pixels.  Timed with device
synchronisation around `--reps` repetitions per window, `--windows` windows per mode, the modes taken in turn inside
every round (drift of the box hits all alike); median, min and max of the windows are reported, in ms per repetition:
  a  whole_scene ... today's evaluation of both networks: two whole-scene infer_cube calls, the label images to the host,
                     CalAccuracy on the list's pixels
  b  evaluator ..... Evaluator.evaluate((engine, None)) on the list + the read-back of the two K x K matrices
  c  contiguous / list_identity ... infer_cube on n consecutive pixels against infer_pixels on the identity list of the
                     same n (spectra by pixel: the same addressing), ONE network: what the indirection alone costs
  d  epoch ......... 78 replayed training steps of 128 + 128 rows, for scale
On a tree without infer_pixels (the parent commit) only a, c's contiguous half and d run.  One JSON line on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmlpl_amd import HyperParams, NetShape, TrainEngine  # noqa: E402
from cmlpl_amd import infer as infer_mod  # noqa: E402
from cmlpl_amd.models import BaseNet2  # noqa: E402
from cmlpl_amd.patches import extract_patches  # noqa: E402
from tools.hyper_tools import CalAccuracy  # noqa: E402

SHAPES = {"B2": (103, 11, 11, 103, 9), "P": (60, 20, 20, 103, 9), "B5": (48, 15, 15, 48, 20)}
DEV = "cuda:0"
ROWS, COLS, NLIST, EPOCH_STEPS = 610, 340, 42776, 78


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="B2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--modes", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    have_list = hasattr(infer_mod, "infer_pixels")
    want = set(args.modes.split(","))
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "infer_pixels": have_list,
           "scene": [ROWS, COLS], "list": NLIST, "pixel_ratio": ROWS * COLS / NLIST, "reps_per_window": args.reps,
           "windows": args.windows, "workloads": {}}
    for name in args.workloads.split(","):
        shape = SHAPES[name]
        Cc, H, W, bands, K = shape
        g = torch.Generator().manual_seed(7)
        cube = torch.randn(ROWS, COLS, Cc, generator=g).to(DEV)
        X = torch.randn(ROWS * COLS, bands, generator=g).to(DEV)
        pix_h = torch.randperm(ROWS * COLS, generator=g)[:NLIST].sort().values
        truth_h = torch.randint(0, K, (NLIST,), generator=g)
        pix, truth = pix_h.to(DEV), truth_h.to(DEV)
        ident = torch.arange(NLIST, dtype=torch.int64, device=DEV)
        bt = btu = 128
        eng = TrainEngine(NetShape(*shape), bt, btu, HyperParams(), device=DEV, seed=1088, hist_rows=16)
        eng.init_params_default(1088)
        # (d) resident splits of 1024 rows by index, the step replayed from its graph
        n = 1024
        lab_pix, unl_pix = (torch.randint(0, ROWS * COLS, (n,), generator=g).to(DEV) for _ in range(2))
        Xl, Yl, Xu = X[lab_pix].contiguous(), torch.randint(0, K, (n,), generator=g).to(DEV), X[unl_pix].contiguous()
        XP, XPu = extract_patches(cube, lab_pix, H), extract_patches(cube, unl_pix, H)
        lp, up = torch.randperm(n, generator=g).to(DEV), torch.randperm(n, generator=g).to(DEV)
        eng.step(XP, Xl, Yl, XPu, Xu, 1, 0, lab_idx=lp[:bt], unl_idx=up[:btu])
        graph = eng.capture(XP, Xl, Yl, XPu, Xu, lp, up, bt, btu, capacity=4096)
        nb = n // bt
        models = []
        for k in range(2):
            m = BaseNet2(num_features=bands, dropout=0.8, num_classes=K, in_channels=Cc, window=H).to(DEV)
            m.load_state_dict(eng.state_dict(k))
            m.eval()
            models.append(m)
        truth_np, pix_np = truth_h.numpy(), pix_h.numpy()

        def whole_scene():
            for m in models:
                pred = infer_mod.infer_cube(m, cube, X).cpu().numpy()
                CalAccuracy(pred[pix_np], truth_np)

        def epoch():
            graph.program([(1, i % nb, (i % nb) * bt, (i % nb) * btu) for i in range(EPOCH_STEPS)])
            for _ in range(EPOCH_STEPS):
                graph.launch()

        modes = {}
        if "a" in want:
            modes["whole_scene"] = whole_scene
        if "c" in want or "c0" in want:                     # (c0: the contiguous half alone, for tree-against-tree runs)
            modes["contiguous"] = lambda: infer_mod.infer_cube(models[0], cube, X, pixel0=0, n=NLIST)
        if "d" in want:
            modes["epoch"] = epoch
        if have_list:
            from cmlpl_amd.evaluate import Evaluator
            ev = Evaluator(NetShape(*shape), cube, X[pix].contiguous(), truth, pix)
            if "b" in want:
                modes["evaluator"] = lambda: ev.evaluate((eng, None)).cpu()
            if "c" in want:
                modes["list_identity"] = lambda: infer_mod.infer_pixels(models[0], cube, X, ident, spec_rows=ident, check=False)
        times = {k: [] for k in modes}
        for run in modes.values():                             # warm every mode
            run()
            run()
        torch.cuda.synchronize()
        for _ in range(args.windows):
            for k, run in modes.items():                       # the modes in turn inside every round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    run()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / args.reps * 1e3)
        out = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in times.items()}
        med = lambda k: out[k]["ms_median"]
        if "whole_scene" in out and "evaluator" in out:
            out["a_over_b"] = med("whole_scene") / med("evaluator")
        if "evaluator" in out and "epoch" in out:
            out["b_over_d"] = med("evaluator") / med("epoch")
        if "contiguous" in out and "list_identity" in out:
            out["list_over_contiguous"] = med("list_identity") / med("contiguous")
        res["workloads"][name] = out
        del graph, eng, XP, XPu
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
