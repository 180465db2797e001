#!/usr/bin/env python3
"""What superpixels and the region vote cost, on one GPU, in one process:
    python scripts/bench_superpixel.py [--scene 610x340] [--classes 9] [--channels 60] [--parent DIR] [--out FILE.json]
  * ``cmlpl_sp_segment`` on a --scene map under a --channels cube (G = 3) at S = 4, 8, 16 and T = 10, between event pairs:
    microseconds per call, and per iteration as (T = 10 minus T = 1) / 9 (medians, min .. max);
  * the two vote calls (``cmlpl_sp_vote_probs`` / ``cmlpl_sp_vote_labels``, every output) over each of those maps;
  * the same definition written in plain torch on the device (nine candidate passes over the whole map, index_add_ for the
    update and the vote) -- what a user would have written without the kernels --, milliseconds;
  * the bytes-once floor: the guide read once from the cube's records (n G 4 bytes useful; n 64-byte lines touched) plus
    T passes over the planar guide and the map, and for the vote n (2 K + 1) 4 bytes, at the HBM rate a float4 copy
    measures on an MI355X (6.29 TB/s);
  * ``superpixel_probs`` behind ``ensemble_cube`` of the two networks of a B2 engine on a synthetic scene of --scene
    pixels against ``ensemble_cube`` alone and ``infer_cube``, taken in turn; milliseconds per scene.
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


def torch_segment(cube, S, m, T, G):
    """the definition in plain torch (fp32, fused or not as torch pleases): the map int64 [n]"""
    rows, cols, _ = cube.shape
    n, dev = rows * cols, cube.device
    g = cube[:, :, :G].reshape(n, G).contiguous()
    ny, nx = -(-rows // S), -(-cols // S)
    N, w = ny * nx, (m * m) / (S * S)
    i = torch.arange(n, device=dev)
    yy, xx = i // cols, i % cols
    pa, pb = yy // S, xx // S
    s = torch.arange(N, device=dev)
    py = torch.clamp((s // nx) * S + S // 2, max=rows - 1)
    px = torch.clamp((s % nx) * S + S // 2, max=cols - 1)
    centres = torch.cat([py[:, None].float(), px[:, None].float(), g[py * cols + px]], 1)
    pos = torch.stack([yy.float(), xx.float()], 1)
    feat = torch.cat([pos, g], 1)
    label = pa * nx + pb
    for _ in range(T):
        best = torch.full((n,), float("inf"), device=dev)
        new = pa * nx + pb
        for da in (-1, 0, 1):
            for db in (-1, 0, 1):
                ca, cb = pa + da, pb + db
                ok = (ca >= 0) & (ca < ny) & (cb >= 0) & (cb < nx)
                cand = torch.where(ok, ca * nx + cb, torch.zeros_like(ca))
                c = centres[cand]
                D = ((g - c[:, 2:]) ** 2).sum(1) + w * ((pos - c[:, :2]) ** 2).sum(1)
                win = ok & (D < best)
                best, new = torch.where(win, D, best), torch.where(win, cand, new)
        label = new
        cnt = torch.zeros(N, device=dev).index_add_(0, label, torch.ones(n, device=dev))
        sums = torch.zeros(N, 2 + G, device=dev).index_add_(0, label, feat)
        centres = torch.where(cnt[:, None] > 0, sums / cnt[:, None].clamp(min=1), centres)
    return label


def torch_vote(seg, p, N):
    sums = torch.zeros(N, p.shape[1], device=p.device).index_add_(0, seg, p)
    cnt = torch.zeros(N, device=p.device).index_add_(0, seg, torch.ones(len(seg), device=p.device))
    q = sums / cnt[:, None]
    return q[seg], q.argmax(1)[seg]


def launches(rows, cols, K, channels, pairs=15, G=3, T=10):
    lib = _lib.load()
    gen = torch.Generator().manual_seed(5)
    n = rows * cols
    p = torch.softmax(2 * torch.randn(n, K, generator=gen), 1).to(DEV)
    hard = p.argmax(1).contiguous()
    # a scene with something to find: blocks of 12 pixels with a guide of their own, and noise
    by, bx = torch.arange(rows) // 12, torch.arange(cols) // 12
    proto = torch.randn(int(by.max()) + 1, int(bx.max()) + 1, channels, generator=gen) * 2
    cube = (proto[by][:, bx] + 0.5 * torch.randn(rows, cols, channels, generator=gen)).to(DEV).contiguous()
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    out, labels = torch.empty(n, K, device=DEV), torch.empty(n, dtype=torch.int64, device=DEV)
    conf, ent = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    res = []
    for S in (4, 8, 16):
        ny, nx = -(-rows // S), -(-cols // S)
        N = ny * nx
        seg = torch.empty(n, dtype=torch.int32, device=DEV)
        cen, cnt = torch.empty(N, 2 + G, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)
        nb = lib.cmlpl_sp_workspace_bytes(rows, cols, G, S)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)

        def seg_call(iters):
            _lib.check("cmlpl_sp_segment", lib.cmlpl_sp_segment(cube.data_ptr(), channels, G, rows, cols, S, 1.0, iters, seg.data_ptr(),
                                                                cen.data_ptr(), cnt.data_ptr(), ws.data_ptr(), nb, st))
        t1 = [t * 1e3 for t in timed(lambda: seg_call(1), pairs)]
        tT = [t * 1e3 for t in timed(lambda: seg_call(T), pairs)]
        vb = lib.cmlpl_sp_vote_workspace_bytes(N, K)
        vws = torch.empty(vb, dtype=torch.uint8, device=DEV)
        sums, vcnt = torch.empty(N, K, dtype=torch.int64, device=DEV), torch.empty(N, dtype=torch.int64, device=DEV)
        sq, sl = torch.empty(N, K, device=DEV), torch.empty(N, dtype=torch.int64, device=DEV)

        def vote_call(fn, src):
            _lib.check(fn, getattr(lib, fn)(seg.data_ptr(), src.data_ptr(), n, K, N, out.data_ptr(), labels.data_ptr(), conf.data_ptr(),
                                            ent.data_ptr(), sums.data_ptr(), vcnt.data_ptr(), sq.data_ptr(), sl.data_ptr(),
                                            vws.data_ptr(), vb, st))
        vp = [t * 1e3 for t in timed(lambda: vote_call("cmlpl_sp_vote_probs", p), pairs)]
        vote_labels_dev = labels.clone()
        vl = [t * 1e3 for t in timed(lambda: vote_call("cmlpl_sp_vote_labels", hard), pairs)]
        tseg = torch_segment(cube, S, 1.0, T, G)
        t_ms = timed(lambda: torch_segment(cube, S, 1.0, T, G), 3, warm=1)
        tv_ms = timed(lambda: torch_vote(tseg, p, N), 5, warm=1)
        agree = float((tseg == seg.long()).float().mean())
        same_vote = float((torch_vote(seg.long(), p, N)[1] == vote_labels_dev).float().mean())
        floor_seg = n * 64 + T * n * (2 * G * 4 + 1 + 2 * 4)            # pack's lines, then per iteration guide + flag twice, map twice
        floor_vote = n * (2 * K + 1) * 4
        res.append(dict(S=S, segments=N, empty=int((cnt == 0).sum()), max_size=int(cnt.max()),
                        segment_T1_us=spread(t1), segment_T10_us=spread(tT),
                        per_iteration_us=(statistics.median(tT) - statistics.median(t1)) / (T - 1),
                        vote_probs_us=spread(vp), vote_labels_us=spread(vl), torch_segment_ms=spread(t_ms), torch_vote_ms=spread(tv_ms),
                        pixels_labelled_as_torch=agree, vote_labels_as_torch=same_vote,
                        floor_segment_bytes=floor_seg, floor_segment_us=floor_seg / HBM_BYTES_PER_S * 1e6,
                        floor_vote_bytes=floor_vote, floor_vote_us=floor_vote / HBM_BYTES_PER_S * 1e6,
                        torch_over_kernels=statistics.median(t_ms) * 1e3 / statistics.median(tT)))
    return dict(scene=[rows, cols], classes=K, channels=channels, guide=G, iters=T, cases=res)


def scene(rows, cols, reps):
    from cmlpl_amd.ensemble import ensemble_cube
    from cmlpl_amd.infer import infer_cube
    from cmlpl_amd.superpixel import Superpixel, superpixel_probs
    eng = TrainEngine(NetShape(*B2), 32, 32, HyperParams(), device=DEV, seed=1088, hist_rows=8)
    eng.init_params_default(1088)
    g = torch.Generator().manual_seed(3)
    cube = torch.randn(rows, cols, B2[0], generator=g).to(DEV)
    X = torch.randn(rows * cols, B2[3], generator=g).to(DEV)
    raw = ensemble_cube((eng, None), cube, X, probs=True)
    modes = {"infer_cube": lambda: infer_cube((eng, 0), cube, X),
             "ensemble_cube_probs": lambda: ensemble_cube((eng, None), cube, X, probs=True),
             "superpixel_probs_S8": lambda: superpixel_probs(raw.probs, cube, Superpixel(8)),
             "superpixel_probs_S4": lambda: superpixel_probs(raw.probs, cube, Superpixel(4)),
             "superpixel_probs_S8_hard": lambda: superpixel_probs(raw.probs, cube, Superpixel(8, vote="hard"), labels=raw.labels)}
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
    res["launch"] = launches(rows, cols, args.classes, args.channels)
    res["B2"] = scene(rows, cols, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
