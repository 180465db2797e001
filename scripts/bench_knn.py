#!/usr/bin/env python3
"""What the kNN evaluation of the embedding costs, on one GPU:
    python scripts/bench_knn.py [--loo 42776] [--queries 207400] [--gallery 4096] [--parent DIR] [--out FILE.json]
  (a) cmlpl_knn alone, event-timed, medians of 7: leave-one-out over --loo rows (PaviaU's labelled test pixels), K = 9,
      k = 10, and --queries rows (a PaviaU scene) against a gallery of --gallery;
  (b) the same definition in plain torch on the device beside it, 4,096 queries at a time: torch.mm in fp32 (rocBLAS),
      masking, topk, gather, scatter_add;
  (c) the floors: the MFMA issue floor 3 * 2 n m 1024 / 2.5 PFLOP/s of the two-piece route, and the bytes-once floor (both
      sides read once, the results written) at the copy rate torch reaches here;
  (d) cmlpl_embed of --loo x 103 bands;
  (e) `--parent DIR` (a checkout of the parent commit with its own built library): plain `bench.py --gpus 1` there and
      here, in alternation, `--bench-reps` times each -- the default path must lie inside the parent's own spread.
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

DEV = "cuda:0"
D = 1024


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(call, reps=7, warm=2):
    """milliseconds per call, each call between two events of its own: the spread of `reps` calls"""
    for _ in range(warm):
        call()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return spread(ms)


def bench_py(tree, steps, warmup):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed:\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def rows_of(n, K, seed):
    """unit rows around K class centroids, as tests/test_gpu_knn.py makes them"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    cent = torch.randn(K, D, generator=torch.Generator(device=DEV).manual_seed(7), device=DEV)
    lab = torch.randint(0, K, (n,), generator=g, device=DEV)
    x = torch.relu(cent[lab] + 3.0 * torch.randn(n, D, generator=g, device=DEV))
    return (x / x.norm(dim=1, keepdim=True)).contiguous(), lab


def torch_knn(q, g, lab, K, k, inv_T, loo, chunk=4096):
    """the definition in plain torch: fp32 GEMM, topk (ties in torch's order), the vote by scatter_add"""
    n = q.shape[0]
    probs = torch.empty(n, K, device=q.device)
    for o in range(0, n, chunk):
        s = torch.mm(q[o:o + chunk], g.t())
        if loo:
            s.diagonal(o).fill_(float("-inf"))
        v, i = s.topk(k, dim=1)
        w = torch.exp((v - v[:, :1]) * inv_T)
        p = torch.zeros(s.shape[0], K, device=q.device).scatter_add_(1, lab[i], w)
        probs[o:o + chunk] = p / w.sum(1, keepdim=True)
    return probs.argmax(1), probs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loo", type=int, default=42776)
    ap.add_argument("--queries", type=int, default=207400)
    ap.add_argument("--gallery", type=int, default=4096)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--T", type=float, default=0.07)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its own built library")
    ap.add_argument("--bench-reps", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"date": time.strftime("%Y-%m-%d"), "script": "scripts/bench_knn.py"}
    if args.parent:
        # first, and in child processes only: this process has not touched the device yet
        runs = {"parent": [], "this": []}
        for _ in range(args.bench_reps):
            runs["parent"].append(bench_py(os.path.abspath(args.parent), args.bench_steps, args.bench_warmup))
            runs["this"].append(bench_py(ROOT, args.bench_steps, args.bench_warmup))
        res["bench_py_ms_per_step"] = {k: dict(spread(v), runs=v) for k, v in runs.items()}
        p, t = res["bench_py_ms_per_step"]["parent"], res["bench_py_ms_per_step"]["this"]
        res["bench_py_inside_parents_spread"] = bool(p["min"] <= t["median"] <= p["max"])
    from cmlpl_amd import knn as KN
    res["device"] = torch.cuda.get_device_name(0)
    K, k, T = args.classes, args.k, args.T
    inv_T = KN.inv_T_of(T)
    big = torch.empty(2 << 30, dtype=torch.uint8, device=DEV)        # (1 GiB each way: past the last-level cache)
    copy_ms = timed(lambda: big[:1 << 30].copy_(big[1 << 30:]))["median"]
    rate = 2 * (1 << 30) / copy_ms                                   # bytes per millisecond, read + write
    del big
    res["copy_GBps"] = rate / 1e6
    cases = {"loo": (args.loo, args.loo, True), "scene": (args.queries, args.gallery, False)}
    res["knn_ms"] = {}
    for name, (n, m, loo) in cases.items():
        g, lab = rows_of(m, K, 1)
        q = g if loo else rows_of(n, K, 2)[0]
        skip = torch.arange(n, dtype=torch.int64, device=DEV) if loo else None
        ws = torch.empty(KN.workspace_bytes(n, m, k), dtype=torch.uint8, device=DEV)
        got = KN.knn(q, g, lab, K, k, T, skip=skip, workspace=ws)
        want = torch_knn(q, g, lab, K, k, inv_T, loo)
        entry = dict(n=n, m=m, K=K, k=k, T=T,
                     kernel=timed(lambda: KN.knn(q, g, lab, K, k, T, skip=skip, workspace=ws)),
                     torch=timed(lambda: torch_knn(q, g, lab, K, k, inv_T, loo)),
                     mfma_floor_ms=3 * 2.0 * n * m * D / 2.5e15 * 1e3,
                     bytes_once_floor_ms=((n if not loo else 0) + m) * D * 4 / rate + n * (K * 4 + 8) / rate,
                     labels_agree=float((got.labels == want[0]).float().mean()),
                     probs_max_diff=float((got.probs - want[1]).abs().max()))
        entry["kernel_below_torch_by_more_than_its_spread"] = bool(
            entry["torch"]["median"] - entry["kernel"]["median"] > entry["torch"]["max"] - entry["torch"]["min"])
        res["knn_ms"][name] = entry
        del q, g, ws
    # (d) the embedding of as many rows as PaviaU's labelled test pixels (103 bands) under one network
    from cmlpl_amd.models import BaseNet2
    net = BaseNet2(num_features=103, dropout=0.8, num_classes=9, in_channels=103, window=11).to(DEV).eval()
    X = torch.randn(args.loo, 103, device=DEV)
    feat = torch.empty(1, args.loo, D, device=DEV)
    norm = torch.empty(1, args.loo, device=DEV)
    res["embed_ms"] = dict(n=args.loo, bands=103, kernel=timed(lambda: KN.embed(net, X, out=(feat, norm))),
                           bytes_once_floor_ms=(X.numel() + feat.numel()) * 4 / rate)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
