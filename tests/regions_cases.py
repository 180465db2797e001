"""The maps the connected-region tests run on (tests/test_regions_host.py, tests/test_gpu_regions.py): patterns chosen for
where a tiled union-find can go wrong -- one component across every tile border, as many components as pixels, one-pixel
paths that wind through many tiles (the longest parent chains), tortuous random clusters near the percolation threshold,
voids, and values up to 2^31 - 1."""
import functools

import numpy as np

PATTERNS = ("constant", "checker", "stripes_h", "stripes_v", "spiral", "comb", "random2", "random9", "smoothed", "voids",
            "all_void", "large_values")


def spiral(rows, cols):
    """a one-pixel-wide path (value 1) that winds inwards, one pixel of background (value 0) between its turns"""
    m = np.zeros((rows, cols), np.int32)
    inside = lambda y, x: 0 <= y < rows and 0 <= x < cols
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y = x = d = 0
    m[0, 0] = 1
    while True:
        for _ in range(2):                              # straight on, or one turn inwards
            dy, dx = dirs[d]
            if inside(y + dy, x + dx) and m[y + dy, x + dx] == 0 and not (inside(y + 2 * dy, x + 2 * dx) and m[y + 2 * dy, x + 2 * dx]):
                break
            d = (d + 1) % 4
        else:
            return m
        y, x = y + dy, x + dx
        m[y, x] = 1


def comb(rows, cols):
    """a spine along the last row and a tooth on every second column: one component whose first pixel is far from most of it"""
    m = np.zeros((rows, cols), np.int32)
    m[rows - 1, :] = 3
    m[:, ::2] = 3
    return m


@functools.lru_cache(maxsize=None)
def smoothed_case(rows, cols, K, G, R, seed=1):
    """(labels int32 [n], truth) of the case builder's map smoothed by the definition (sigma_s 2, sigma_r 1)"""
    from tests.test_smooth_host import case, smooth_def
    p, cube, Y = case(rows, cols, K, G, seed)
    lab = smooth_def(p, cube[:, :, :G], rows, cols, R, 2.0, 1.0)["label"].astype(np.int32)
    lab.setflags(write=False)
    return lab, Y


def pattern(name, rows, cols, seed=0):
    """the int32 map [rows * cols] of a pattern"""
    rng = np.random.default_rng(seed)
    n = rows * cols
    yy, xx = np.divmod(np.arange(n), cols)
    if name == "constant":
        m = np.full(n, 5)
    elif name == "checker":
        m = (yy + xx) % 2
    elif name == "stripes_h":
        m = yy % 2
    elif name == "stripes_v":
        m = xx % 2
    elif name == "spiral":
        m = spiral(rows, cols)
    elif name == "comb":
        m = comb(rows, cols)
    elif name == "random2":
        m = (rng.random(n) < 0.59).astype(np.int32)
    elif name == "random9":
        m = rng.integers(0, 9, n)
    elif name == "smoothed":
        m = smoothed_case(rows, cols, 9, 3, 2)[0] if rows * cols > 64 else rng.integers(0, 3, n)
    elif name == "voids":
        m = np.where(rng.random(n) < 0.15, -1 - rng.integers(0, 3, n), (rng.random(n) < 0.6).astype(np.int64))
    elif name == "all_void":
        m = np.full(n, -1)
    elif name == "large_values":
        m = np.repeat(rng.choice([2 ** 31 - 1, 2 ** 24, 2 ** 24 - 1, 123456789, 0], (n + 2) // 3), 3)[:n]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(np.asarray(m).reshape(-1).astype(np.int32))
