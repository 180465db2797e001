#!/usr/bin/env python3
"""What connected components and the sieve cost, on one GPU, in one process:
    python scripts/bench_regions.py [--scene 610x340] [--parent DIR] [--out FILE.json]
  * ``cmlpl_cc_label`` alone (comp, size, id, M) on a --scene map, between event pairs, microseconds per call (medians,
    min .. max): a smoothed 9-class map from the tests' case builder, a constant map, a one-pixel spiral, and a K = 2 random
    map at density 0.59 (tortuous clusters near the percolation threshold);
  * ``cmlpl_cc_sieve`` at min_size 4 with 1 and 4 passes on the smoothed and the random map;
  * ``connect_segments`` (the sieve and the ids; its one word read back included) behind ``cmlpl_sp_segment`` at S = 4 / 8 / 16;
  * the bytes-once floor of the labelling -- the map read, comp written: 8 n bytes -- at the HBM rate a float4 copy measures on
    an MI355X (6.29 TB/s);
  * ``scipy.ndimage.label`` (one value's mask) on the host for scale, if scipy imports;
  * the sieve stage (``sieve`` of the labels with the conf gather) beside ``ensemble_cube`` of the two networks of a B2 engine
    on a synthetic scene of --scene pixels, taken in turn; milliseconds per scene.
`--parent DIR` (a checkout of the parent commit with its own built library): plain `bench.py --gpus 1` there and here, in
alternation, `--bench-reps` times each -- the default step executes no new code and must lie inside the parent's own spread.
One JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmlpl_amd import _lib  # noqa: E402
from cmlpl_amd.regions import Sieve, connect_segments, sieve  # noqa: E402
from scripts.bench_superpixel import B2, DEV, HBM_BYTES_PER_S, bench_py, spread, timed  # noqa: E402


def maps(rows, cols):
    from tests.regions_cases import pattern, smoothed_case
    return {"smoothed_K9": np.ascontiguousarray(smoothed_case(rows, cols, 9, 3, 2)[0]), "constant": pattern("constant", rows, cols),
            "spiral": pattern("spiral", rows, cols), "random2_p0.59": pattern("random2", rows, cols, 5)}


def launches(rows, cols, pairs=15):
    lib = _lib.load()
    n = rows * cols
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    nb = lib.cmlpl_cc_workspace_bytes(rows, cols)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    comp, size, ident, out = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(4))
    M, stats = torch.empty(1, dtype=torch.int32, device=DEV), torch.empty(16, 4, dtype=torch.int32, device=DEV)
    res = {"scene": [rows, cols], "floor_bytes": 8 * n, "floor_us": 8 * n / HBM_BYTES_PER_S * 1e6, "maps": {}}
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for name, v in maps(rows, cols).items():
        vt = torch.from_numpy(v).to(DEV)

        def label(full=True):
            _lib.check("cmlpl_cc_label", lib.cmlpl_cc_label(vt.data_ptr(), rows, cols, 4, comp.data_ptr(), size.data_ptr() if full else None,
                                                            ident.data_ptr() if full else None, M.data_ptr() if full else None,
                                                            ws.data_ptr(), nb, st))

        def sieve_call(passes):
            _lib.check("cmlpl_cc_sieve", lib.cmlpl_cc_sieve(vt.data_ptr(), rows, cols, 4, 4, passes, out.data_ptr(), stats.data_ptr(),
                                                            None, 0, None, ws.data_ptr(), nb, st))
        case = {"label_us": spread([t * 1e3 for t in timed(label, pairs)]),
                "label_comp_only_us": spread([t * 1e3 for t in timed(lambda: label(False), pairs)]), "components": int(M.item())}
        if name in ("smoothed_K9", "random2_p0.59"):
            for passes in (1, 4):
                case["sieve_%dpass_us" % passes] = spread([t * 1e3 for t in timed(lambda: sieve_call(passes), pairs)])
            case["sieve_stats"] = stats[:4].cpu().tolist()
        if ndimage is not None:
            t0 = time.perf_counter()
            ndimage.label((v == v[0]).reshape(rows, cols))
            case["scipy_label_one_value_ms"] = (time.perf_counter() - t0) * 1e3
        res["maps"][name] = case
    return res


def segments(rows, cols, channels=60, pairs=9):
    from cmlpl_amd.superpixel import Superpixel, segment
    gen = torch.Generator().manual_seed(5)
    by, bx = torch.arange(rows) // 12, torch.arange(cols) // 12
    proto = torch.randn(int(by.max()) + 1, int(bx.max()) + 1, channels, generator=gen) * 2
    cube = (proto[by][:, bx] + 0.5 * torch.randn(rows, cols, channels, generator=gen)).to(DEV).contiguous()
    res = []
    for S in (4, 8, 16):
        segs = segment(cube, Superpixel(S))
        ids, M = connect_segments(segs.seg, rows, cols, max(1, S * S // 4))
        res.append(dict(S=S, segments=segs.N, connected_segments=M, segment_us=spread([t * 1e3 for t in timed(lambda: segment(cube, Superpixel(S)), pairs)]),
                        connect_segments_us=spread([t * 1e3 for t in timed(lambda: connect_segments(segs.seg, rows, cols, max(1, S * S // 4)), pairs)])))
    return res


def scene(rows, cols, reps):
    from cmlpl_amd import HyperParams, NetShape, TrainEngine
    from cmlpl_amd.ensemble import ensemble_cube
    eng = TrainEngine(NetShape(*B2), 32, 32, HyperParams(), device=DEV, seed=1088, hist_rows=8)
    eng.init_params_default(1088)
    g = torch.Generator().manual_seed(3)
    cube = torch.randn(rows, cols, B2[0], generator=g).to(DEV)
    X = torch.randn(rows * cols, B2[3], generator=g).to(DEV)
    raw = ensemble_cube((eng, None), cube, X, probs=True)
    modes = {"ensemble_cube_probs": lambda: ensemble_cube((eng, None), cube, X, probs=True),
             "sieve_stage_4pass": lambda: sieve(raw.labels, rows, cols, Sieve(4), probs=raw.probs)}
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
            print("bench.py ms/step: parent %.3f, this %.3f" % (runs["parent"][-1], runs["this"][-1]), file=sys.stderr, flush=True)
        res["bench_py_ms_per_step"] = {k: dict(spread(v), runs=v) for k, v in runs.items()}
        p, t = res["bench_py_ms_per_step"]["parent"], res["bench_py_ms_per_step"]["this"]
        res["bench_py_inside_parents_spread"] = bool(p["min"] <= t["median"] <= p["max"])
    res["device"] = torch.cuda.get_device_name(0)
    rows, cols = (int(v) for v in args.scene.split("x"))
    res["launch"] = launches(rows, cols)
    res["connect_segments"] = segments(rows, cols)
    res["B2"] = scene(rows, cols, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
