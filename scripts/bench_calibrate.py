#!/usr/bin/env python3
"""What calibration costs, on one GPU:
    python scripts/bench_calibrate.py [--rows 207400] [--classes 9] [--parent DIR] [--out FILE.json]
  * each launch alone over a probability map of --rows x --classes (a PaviaU scene: 207,400 x 9), medians of event-timed
    bursts: cmlpl_reliability at 15 and at 1024 bins, cmlpl_temper_probs with every output, cmlpl_nll_temps at 64 candidates;
  * the same definitions in plain torch on the device beside them (binning by bucketize + bincount, softmax of beta log p,
    a [rows, 64, K] log-sum-exp);
  * the bytes-once floor of each: what it must read and write, at the copy rate torch reaches on the same buffers;
  * fit_temperature end to end (two launches of 64 candidates, the read-backs between them) on 42,776 listed rows;
  * `--parent DIR` (a checkout of the parent commit with its own built library): plain `bench.py --gpus 1` there and here,
    in alternation, `--bench-reps` times each -- the default path must lie inside the parent's own spread.
One JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cmlpl_amd import calibrate as cal  # noqa: E402

DEV = "cuda:0"


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(call, pairs=15, burst=20):
    """microseconds per call: `burst` calls between two events, the median of `pairs` such bursts"""
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
    return spread(us)


def bench_py(tree, steps, warmup):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed:\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def torch_reliability(p, truth, bins):
    """the counters' definition in plain torch (float sums instead of fixed point)"""
    K = p.shape[1]
    conf, label = p.max(1)
    known = (truth >= 0) & (truth < K)
    t = truth.clamp(0, K - 1)
    b = (conf * float(bins)).to(torch.int64).clamp(0, bins - 1)
    hit = (label == t) & known
    w = known.to(torch.float32)
    count = torch.bincount(b, weights=w, minlength=bins)
    hits = torch.bincount(b, weights=hit.to(torch.float32), minlength=bins)
    csum = torch.bincount(b, weights=conf * w, minlength=bins)
    pt = p.gather(1, t[:, None])[:, 0]
    nll = -(torch.log(pt) * w).sum()
    brier = (((p - torch.nn.functional.one_hot(t, K)) ** 2).sum(1) * w).sum()
    return count, hits, csum, nll, brier


def torch_temper(p, beta):
    q = torch.softmax(beta * torch.log(p), 1)
    conf, label = q.max(1)
    ent = -(torch.where(q > 0, q * torch.log(q), torch.zeros_like(q))).sum(1)
    return q, label, conf, ent


def torch_nll_temps(p, truth, betas):
    l = torch.log(p)
    z = betas[None, :, None] * l[:, None, :]                       # [rows, S, K]
    return (torch.logsumexp(z, 2) - betas[None, :] * l.gather(1, truth[:, None])).sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=207400)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--fit-rows", type=int, default=42776)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its own built library")
    ap.add_argument("--bench-reps", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"date": time.strftime("%Y-%m-%d"), "rows": args.rows, "classes": args.classes}
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
    n, K = args.rows, args.classes
    g = torch.Generator().manual_seed(1088)
    z0 = torch.randn(n, K, generator=g)
    p = torch.softmax(2 * z0, 1).to(DEV)                            # over-confident by a factor 2
    truth = torch.multinomial(torch.softmax(z0, 1), 1, generator=g)[:, 0].to(DEV)
    betas = cal.coarse_betas()
    dbetas = torch.from_numpy(betas).to(DEV)
    out, lab = torch.empty_like(p), torch.empty(n, dtype=torch.int64, device=DEV)
    conf, ent = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    from cmlpl_amd import _lib
    import ctypes as C
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    blocks = {b: torch.zeros(cal.rel_size(b), dtype=torch.int64, device=DEV) for b in (15, 1024)}
    sums = torch.zeros(2, 64, dtype=torch.int64, device=DEV)
    cb = (C.c_float * 64)(*betas.tolist())
    launches = {
        "reliability_15": lambda: lib.cmlpl_reliability(p.data_ptr(), K, None, truth.data_ptr(), n, 15, blocks[15].data_ptr(), st),
        "reliability_1024": lambda: lib.cmlpl_reliability(p.data_ptr(), K, None, truth.data_ptr(), n, 1024, blocks[1024].data_ptr(), st),
        "temper_probs": lambda: lib.cmlpl_temper_probs(p.data_ptr(), n, K, 0.4926, out.data_ptr(), lab.data_ptr(), conf.data_ptr(),
                                                       ent.data_ptr(), st),
        "nll_temps_64": lambda: lib.cmlpl_nll_temps(p.data_ptr(), K, None, truth.data_ptr(), n, cb, 64, sums.data_ptr(), st),
    }
    plain = {
        "reliability_15": lambda: torch_reliability(p, truth, 15),
        "reliability_1024": lambda: torch_reliability(p, truth, 1024),
        "temper_probs": lambda: torch_temper(p, 0.4926),
        "nll_temps_64": lambda: torch_nll_temps(p, truth, dbetas),
    }
    # the bytes-once floor: what a launch must read and write, at the rate a device copy of the map reaches here
    copy_us = timed(lambda: out.copy_(p))["median"]
    rate = 2 * p.numel() * 4 / copy_us                              # bytes per microsecond, read + write
    moved = {"reliability_15": p.numel() * 4 + n * 8, "reliability_1024": p.numel() * 4 + n * 8,
             "temper_probs": 2 * p.numel() * 4 + n * 16, "nll_temps_64": p.numel() * 4 + n * 8}
    res["copy_GBps"] = rate / 1e3
    res["launch_us"] = {}
    for k in launches:
        assert launches[k]() == 0
        res["launch_us"][k] = dict(kernel=timed(launches[k]), torch=timed(plain[k], pairs=7, burst=5),
                                   bytes_once_floor_us=moved[k] / rate)
    # agreement of what was timed (the torch forms use float sums: compared loosely)
    r = cal.reliability(p, truth, None, 15)
    tc = torch_reliability(p, truth, 15)
    res["agree"] = dict(count=bool((tc[0].cpu().numpy() == r.count).all()), nll=[float(tc[3]) / n, r.nll], ece=r.ece)
    # fit_temperature end to end on a list of rows
    m = min(args.fit_rows, n)
    rows = torch.randperm(n, generator=g)[:m].to(DEV)
    tl = truth[rows].contiguous()
    fit = []
    cal.fit_temperature(p, tl, rows)
    for _ in range(9):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T = cal.fit_temperature(p, tl, rows)
        fit.append((time.perf_counter() - t0) * 1e3)
    res["fit_temperature"] = dict(rows=m, T=T[0], nll_before=T[1], nll_after=T[2], ms=spread(fit))
    after = cal.reliability(cal.temper_probs(p, T[0]).probs, truth, None, 15)
    res["ece_before_after"] = [r.ece, after.ece]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
