#!/usr/bin/env python3
"""The cross-pseudo-supervision step against the CMLPL step of the same build on one GPU, interleaved in one process:
    python scripts/bench_cps.py [--workloads B2,P] [--steps 100] [--windows 7] [--out FILE.json]
For each workload at 128 + 128 rows, by index over resident splits of --rows rows (seeded synthetic data), eager and
replayed from the captured graph:
  * cps          -- TrainEngine(method="cps");
  * cmlpl_fresh  -- the CMLPL step in the benchmark's state (thr = 1: no unlabelled row passes the threshold, the
                    backward skips their zero-gradient rows);
  * cmlpl_thr0   -- the CMLPL step with thr = 0: every row carries a gradient, which is what a CPS step always is.
`--windows` timed windows of `--steps` steps per mode, the modes taken in turn inside every round (drift of the box hits
all alike); median, min and max of the windows are reported.  Then, eager, with cmlpl_timing_begin/_end: the loss
launches alone in microseconds (cps_loss | loss = pair_exp + loss_rows, loss_graph, loss_dfeat) and the timed launches
per step of both methods (the 4-byte memset in front of the CPS loss launch is not a timed launch).  One JSON line."""
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

SHAPES = {"B2": (103, 11, 11, 103, 9), "P": (60, 20, 20, 103, 9), "B5": (48, 15, 15, 48, 20)}
DEV = "cuda:0"
KINDS = {"cps": dict(method="cps", thr=1.0), "cmlpl_fresh": dict(method="cmlpl", thr=1.0),
         "cmlpl_thr0": dict(method="cmlpl", thr=0.0)}


def make_mode(shape, bt, btu, rows_split, kind, graph, data):
    XP, X, Y, XPu, Xu, lp, up = data
    eng = TrainEngine(NetShape(*shape), bt, btu, HyperParams(thr=KINDS[kind]["thr"]), device=DEV, seed=1088, hist_rows=16,
                      method=KINDS[kind]["method"])
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


def timed(run, steps, mask):
    nk = len(_lib.KERNEL_NAMES)
    ms, cnt = (C.c_double * nk)(), (C.c_int64 * nk)()
    lib = _lib.load()
    _lib.check("cmlpl_timing_begin", lib.cmlpl_timing_begin(mask, 64 * steps))
    run(steps)
    _lib.check("cmlpl_timing_end", lib.cmlpl_timing_end(ms, cnt))
    return {nm: (ms[i] / cnt[i] * 1e3, cnt[i] / steps) for i, nm in enumerate(_lib.KERNEL_NAMES) if cnt[i]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="B2,P")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1024, help="rows per resident split")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "steps_per_window": args.steps,
           "windows": args.windows, "workloads": {}}
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
        for kind in KINDS:
            for gr in (False, True):
                modes[kind + ("_graph" if gr else "_eager")] = make_mode(shape, bt, btu, n, kind, gr, data)
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
        loss_ids = ("cps_loss", "loss", "loss_graph", "loss_dfeat")
        mask = sum(1 << _lib.KERNEL_NAMES.index(k) for k in loss_ids)
        out["loss_us"] = {kind: {k: round(v[0], 2) for k, v in timed(modes[kind + "_eager"][1], 50, mask).items()}
                          for kind in KINDS}
        out["timed_launches_per_step"] = {
            kind: sum(v[1] for v in timed(modes[kind + "_eager"][1], 4, (1 << len(_lib.KERNEL_NAMES)) - 1).values())
            for kind in ("cps", "cmlpl_fresh")}
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
