#!/usr/bin/env python3
"""What the region graph costs, on one GPU, in one process:
    python scripts/bench_regiongraph.py [--scene 610x340] [--parent DIR] [--out FILE.json]
On a --scene of 103-band spectra and a 60-channel cube, over the connected superpixel map at S = 4 / 8 / 16 (``--sp_connect``),
between event pairs, microseconds per call (medians, min .. max of 15):
  * ``cmlpl_rg_pool`` at B = 103, and the same call at B = 1 -- its eight launches with next to no band work, an upper bound
    of the pixel-index step (histogram, scan, scatter) inside it;
  * ``cmlpl_rg_adjacency`` at A = 8, ``cmlpl_rg_lists`` at k = 8, A = 8;
  * what they feed: ``embed`` of the mean spectra + ``knn`` (k = 8, leave-one-out) + ``build_graph`` + ``propagate`` (20
    iterations, K = 9);
  * the same definitions in plain torch on the device: ``index_add_`` of the spectra for the pool (fp32: not the bytes of the
    definition), a sort of packed (s, t) pairs with ``unique_consecutive`` for the adjacency counts (no top-A cut);
  * the bytes-once floors at the 6.29 TB/s a float4 copy reaches on an MI355X: ``n B 4`` bytes for the pool, the map read
    twice (``8 n`` bytes) for the adjacency;
  * the stage in total (``region_graph`` + ``region_propagate`` behind a vote) beside ``ensemble_cube`` of the two networks of
    a B2 engine, taken in turn; milliseconds per scene.
`--parent DIR` (a checkout of the parent commit with its own built library): plain `bench.py --gpus 1` there and here, in
alternation, `--bench-reps` times each -- the default step executes no new code and must lie inside the parent's own spread.
One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cmlpl_amd import _lib  # noqa: E402
from cmlpl_amd.regiongraph import RegionGraph, adjacency, merge_lists, pool, region_graph, region_propagate  # noqa: E402
from scripts.bench_superpixel import B2, DEV, HBM_BYTES_PER_S, bench_py, spread, timed  # noqa: E402


def torch_pool(ids, M, X):
    keep = (ids >= 0) & (ids < M) & (torch.isfinite(X) & (X.abs() <= 256)).all(1)
    at = ids[keep].long()
    sums = torch.zeros(M, X.shape[1], device=X.device).index_add_(0, at, X[keep])
    cnt = torch.zeros(M, device=X.device).index_add_(0, at, torch.ones(len(at), device=X.device))
    return sums / cnt.clamp(min=1)[:, None]


def torch_adjacency(ids, M, rows, cols):
    v = ids.view(rows, cols).long()
    a = torch.cat([v[:, :-1].reshape(-1), v[:-1, :].reshape(-1)])
    b = torch.cat([v[:, 1:].reshape(-1), v[1:, :].reshape(-1)])
    keep = (a >= 0) & (a < M) & (b >= 0) & (b < M) & (a != b)
    a, b = a[keep], b[keep]
    packed = torch.cat([a * M + b, b * M + a]).sort()[0]
    return torch.unique_consecutive(packed, return_counts=True)


def launches(rows, cols, bands=103, channels=60, pairs=15, K=9):
    from cmlpl_amd import HyperParams, NetShape, TrainEngine
    from cmlpl_amd.knn import embed, knn
    from cmlpl_amd.labelprop import build_graph, propagate
    from cmlpl_amd.regions import connect_segments
    from cmlpl_amd.superpixel import Superpixel, segment
    lib = _lib.load()
    n = rows * cols
    gen = torch.Generator().manual_seed(5)
    by, bx = torch.arange(rows) // 12, torch.arange(cols) // 12
    proto = torch.randn(int(by.max()) + 1, int(bx.max()) + 1, channels, generator=gen) * 2
    cube = (proto[by][:, bx] + 0.5 * torch.randn(rows, cols, channels, generator=gen)).to(DEV).contiguous()
    sproto = torch.randn(int(by.max()) + 1, int(bx.max()) + 1, bands, generator=gen)
    X = (sproto[by][:, bx] + 0.3 * torch.randn(rows, cols, bands, generator=gen)).reshape(n, bands).to(DEV).contiguous()
    eng = TrainEngine(NetShape(*B2), 32, 32, HyperParams(), device=DEV, seed=1088, hist_rows=8)
    eng.init_params_default(1088)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    us = lambda fn: spread([t * 1e3 for t in timed(fn, pairs)])
    res = {"scene": [rows, cols], "bands": bands, "pool_floor_us": n * bands * 4 / HBM_BYTES_PER_S * 1e6,
           "adjacency_floor_us": 8 * n / HBM_BYTES_PER_S * 1e6, "maps": []}
    for S in (4, 8, 16):
        ids, M = connect_segments(segment(cube, Superpixel(S)).seg, rows, cols, max(1, S * S // 4))
        nb = lib.cmlpl_rg_workspace_bytes(rows, cols, M, 8)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        mean, cnt = torch.empty(M, bands, device=DEV), torch.empty(M, dtype=torch.int64, device=DEV)
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=DEV)
        adj_idx, adj_len, deg, boundary = i32(M, 8), i32(M, 8), i32(M), i32(M)

        def pool_call(B):
            _lib.check("cmlpl_rg_pool", lib.cmlpl_rg_pool(ids.data_ptr(), rows, cols, M, X.data_ptr(), bands, B, mean.data_ptr(),
                                                          cnt.data_ptr(), None, ws.data_ptr(), nb, st))

        def adj_call():
            _lib.check("cmlpl_rg_adjacency", lib.cmlpl_rg_adjacency(ids.data_ptr(), rows, cols, M, 8, adj_idx.data_ptr(), adj_len.data_ptr(),
                                                                    deg.data_ptr(), boundary.data_ptr(), ws.data_ptr(), nb, st))
        case = dict(S=S, regions=M, pool_us=us(lambda: pool_call(bands)), pool_B1_us=us(lambda: pool_call(1)), adjacency_us=us(adj_call))
        pooled, adj = pool(ids, M, X), adjacency(ids, M, rows, cols, 8)
        feat = embed((eng, 0), pooled.mean)[0]
        skip = torch.arange(M, dtype=torch.int64, device=DEV)
        nn = knn(feat, feat, None, 0, 8, skip=skip)
        case["lists_us"] = us(lambda: merge_lists(feat, nn.nbr_idx, nn.nbr_sim, adj.adj_idx))
        nbr_idx, nbr_sim = merge_lists(feat, nn.nbr_idx, nn.nbr_sim, adj.adj_idx)
        Y = torch.softmax(2 * torch.randn(M, K, generator=gen), 1).to(DEV)

        def fed():
            f = embed((eng, 0), pooled.mean)[0]
            r = knn(f, f, None, 0, 8, skip=skip)
            propagate(build_graph(*merge_lists(f, r.nbr_idx, r.nbr_sim, adj.adj_idx), 3), Y, 0.5, 20)
        case["embed_knn_lists_graph_propagate_us"] = us(fed)
        case["torch_pool_index_add_us"] = us(lambda: torch_pool(ids, M, X))
        case["torch_adjacency_sort_us"] = us(lambda: torch_adjacency(ids, M, rows, cols))
        graph = build_graph(nbr_idx, nbr_sim, 3)
        case.update(truncated=int((adj.deg > 8).sum()), max_deg=int(adj.deg.max()), edges=graph.edges(),
                    max_in_degree=graph.max_in_degree(), max_region=int(pooled.cnt.max()))
        res["maps"].append(case)
    return res


def scene(rows, cols, reps):
    from cmlpl_amd import HyperParams, NetShape, TrainEngine
    from cmlpl_amd.ensemble import ensemble_cube
    from cmlpl_amd.superpixel import Superpixel, superpixel_probs
    eng = TrainEngine(NetShape(*B2), 32, 32, HyperParams(), device=DEV, seed=1088, hist_rows=8)
    eng.init_params_default(1088)
    g = torch.Generator().manual_seed(3)
    cube = torch.randn(rows, cols, B2[0], generator=g).to(DEV)
    X = torch.randn(rows * cols, B2[3], generator=g).to(DEV)
    raw = ensemble_cube((eng, None), cube, X, probs=True)
    cfg = RegionGraph()
    modes = {"ensemble_cube_probs": lambda: ensemble_cube((eng, None), cube, X, probs=True)}
    for S in (4, 8, 16):
        vote = superpixel_probs(raw.probs, cube, Superpixel(S, connect=True))

        def stage(vote=vote):
            rg = region_graph(vote.connected, vote.M, rows, cols, X, [(eng, 0), (eng, 1)], cfg)
            return region_propagate(rg, vote.seg_probs, cfg)
        modes["region_graph_stage_S%d" % S] = stage
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="610x340")
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
            print("bench.py ms/step: parent %.4f, this %.4f" % (runs["parent"][-1], runs["this"][-1]), file=sys.stderr, flush=True)
        res["bench_py_ms_per_step"] = {k: dict(spread(v), runs=v) for k, v in runs.items()}
        p, t = res["bench_py_ms_per_step"]["parent"], res["bench_py_ms_per_step"]["this"]
        res["bench_py_inside_parents_spread"] = bool(p["min"] <= t["median"] <= p["max"])
    res["device"] = torch.cuda.get_device_name(0)
    rows, cols = (int(v) for v in args.scene.split("x"))
    res["launch"] = launches(rows, cols)
    res["B2"] = scene(rows, cols, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
