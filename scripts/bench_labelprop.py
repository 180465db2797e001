#!/usr/bin/env python3
"""What label propagation over the embedding's kNN graph costs, on one GPU:
    python scripts/bench_labelprop.py [--nodes 42821] [--k 10] [--classes 9] [--iters 50] [--parent DIR] [--out FILE.json]
  (a) the graph: knn_graph (the leave-one-out search) and cmlpl_lp_graph, event-timed, medians of 7, at PaviaU's shape
      (42,776 labelled test pixels + 45 training pixels, k = 10);
  (b) one iteration (cmlpl_lp_propagate with every optional output NULL, 1 and --iters iterations: the difference per
      iteration) and the whole call with its finish;
  (c) the hub graph of tests/lp_util.py scaled to the same n: random lists, node 0 in every other row -- one group walks a
      reverse list of n - 1 entries (the skew pitfall of a one-group-per-destination pass);
  (d) beside them the same definition in plain torch on the device over the same edges -- index_add_ and a CSR sparse mm --
      and the bytes-once floor per iteration, list entries x (4 K + 8) bytes at the copy rate torch reaches here;
  (e) `--parent DIR` (a checkout of the parent commit with its own built library): plain `bench.py --gpus 1` there and
      here, in alternation, `--bench-reps` times each -- the default path executes no new code and must lie inside the
      parent's own spread.
One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402
from bench_knn import DEV, bench_py, rows_of, spread, timed  # noqa: E402


def hub_lists(n, k, seed=0):
    """random lists, the hub (node 0) at a random rank of every other row, similarities U(-0.2, 1) descending, a tenth of the
    rows cut by pads behind the hub"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    idx = torch.randint(1, n, (n, k), generator=g, device=DEV, dtype=torch.int32)
    at = torch.randint(0, k, (n,), generator=g, device=DEV)
    cut = torch.where(torch.rand(n, generator=g, device=DEV) < 0.1, torch.randint(1, max(k, 2), (n,), generator=g, device=DEV),
                      torch.full((n,), k, device=DEV))
    at = torch.minimum(at, cut - 1)
    idx[torch.arange(1, n, device=DEV), at[1:]] = 0
    sim = (torch.rand(n, k, generator=g, device=DEV) * 1.2 - 0.2).sort(dim=1, descending=True).values
    pad = torch.arange(k, device=DEV)[None, :] >= cut[:, None]
    return torch.where(pad, torch.full_like(idx, -1), idx).contiguous(), torch.where(pad, torch.full_like(sim, float("-inf")), sim).contiguous()


def edge_list(graph):
    """(dst, src, coef) of every list entry of the graph: forward entries, then reverse ones"""
    n, k, E = graph.n, graph.k, graph.edges()
    fwd = graph.fwd_dst.reshape(-1) >= 0
    rows = torch.arange(n, device=DEV).repeat_interleave(k)
    owner = torch.arange(n, device=DEV).repeat_interleave(graph.in_deg.long())
    return (torch.cat([rows[fwd], owner]), torch.cat([graph.fwd_dst.reshape(-1)[fwd].long(), graph.rev_src[:E].long()]),
            torch.cat([graph.fwd_coef.reshape(-1)[fwd], graph.rev_coef[:E]]))


def measure(lib, graph, Y, alpha, iters):
    n, K = Y.shape
    F, tmp = torch.empty_like(Y), torch.empty_like(Y)
    probs, labels = torch.empty_like(Y), torch.empty(n, dtype=torch.int64, device=DEV)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bare = lambda it: lib.cmlpl_lp_propagate(graph.buf.data_ptr(), n, graph.k, Y.data_ptr(), K, alpha, it, None, F.data_ptr(),
                                             tmp.data_ptr(), None, None, None, None, None, st())
    full = lambda: lib.cmlpl_lp_propagate(graph.buf.data_ptr(), n, graph.k, Y.data_ptr(), K, alpha, iters, None, F.data_ptr(),
                                          tmp.data_ptr(), probs.data_ptr(), labels.data_ptr(), None, None, None, st())
    assert bare(1) == 0 and full() == 0
    one, many, whole = timed(lambda: bare(1)), timed(lambda: bare(iters)), timed(full)
    dst, src, coef = edge_list(graph)
    beta = 1.0 - alpha
    S = torch.sparse_coo_tensor(torch.stack([dst, src]), coef, (n, n)).coalesce().to_sparse_csr()

    def by_index_add(it):
        G = Y
        for _ in range(it):
            G = alpha * torch.zeros_like(Y).index_add_(0, dst, coef[:, None] * G[src]) + beta * Y
        return G

    def by_spmm(it):
        G = Y
        for _ in range(it):
            G = alpha * (S @ G) + beta * Y
        return G

    ref = by_index_add(iters)
    try:
        spmm = timed(lambda: by_spmm(iters), reps=5, warm=1)
    except RuntimeError as e:                 # (a torch build without CSR products on this device)
        spmm = str(e)[:200]
    entries = int(dst.numel())
    return dict(n=n, k=graph.k, K=K, iters=iters, list_entries=entries, max_in_degree=graph.max_in_degree(),
                one_iteration_call=one, iterations_call=many, per_iteration_ms=(many["median"] - one["median"]) / max(iters - 1, 1),
                propagate_with_finish=whole, torch_index_add=timed(lambda: by_index_add(iters), reps=5, warm=1),
                torch_spmm=spmm, max_diff_to_torch=float((F - ref).abs().max()),
                max_F=float(ref.abs().max()), entries=entries)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=42776 + 45)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--alpha", type=float, default=0.99)
    ap.add_argument("--gamma", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its own built library")
    ap.add_argument("--bench-reps", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"date": time.strftime("%Y-%m-%d"), "script": "scripts/bench_labelprop.py"}
    if args.parent:
        # first, and in child processes only: this process has not touched the device yet
        runs = {"parent": [], "this": []}
        for _ in range(args.bench_reps):
            runs["parent"].append(bench_py(os.path.abspath(args.parent), args.bench_steps, args.bench_warmup))
            runs["this"].append(bench_py(ROOT, args.bench_steps, args.bench_warmup))
        res["bench_py_ms_per_step"] = {k: dict(spread(v), runs=v) for k, v in runs.items()}
        p, t = res["bench_py_ms_per_step"]["parent"], res["bench_py_ms_per_step"]["this"]
        res["bench_py_inside_parents_spread"] = bool(p["min"] <= t["median"] <= p["max"])
    from cmlpl_amd import _lib, labelprop as LP
    lib = _lib.load()
    res["device"] = torch.cuda.get_device_name(0)
    n, k, K = args.nodes, args.k, args.classes
    big = torch.empty(2 << 30, dtype=torch.uint8, device=DEV)        # (1 GiB each way: past the last-level cache)
    copy_ms = timed(lambda: big[:1 << 30].copy_(big[1 << 30:]))["median"]
    rate = 2 * (1 << 30) / copy_ms                                   # bytes per millisecond, read + write
    del big
    res["copy_GBps"] = rate / 1e6
    seeds = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    seeds[:5 * K] = torch.arange(5 * K, device=DEV) % K              # five per class, in front: the training pixels
    Y = LP.one_hot_seeds(seeds, K)
    feat, _ = rows_of(n, K, 1)
    idx, sim = LP.knn_graph(feat, k)
    res["knn_graph_ms"] = timed(lambda: LP.knn_graph(feat, k))
    res["lp_graph_ms"] = timed(lambda: LP.build_graph(idx, sim, args.gamma))
    graph = LP.build_graph(idx, sim, args.gamma)
    res["embedding"] = measure(lib, graph, Y, args.alpha, args.iters)
    hidx, hsim = hub_lists(n, k)
    res["hub_lp_graph_ms"] = timed(lambda: LP.build_graph(hidx, hsim, args.gamma))
    res["hub"] = measure(lib, LP.build_graph(hidx, hsim, args.gamma), Y, args.alpha, args.iters)
    for name in ("embedding", "hub"):
        e = res[name]
        e["bytes_once_floor_ms_per_iteration"] = e.pop("entries") * (4 * K + 8) / rate
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
