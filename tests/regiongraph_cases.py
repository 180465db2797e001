"""What the region-graph tests share (tests/test_regiongraph_host.py, tests/test_gpu_regiongraph.py): the maps beyond
tests/regions_cases.py -- pixel ids, component ids, the hub map --, and the seeded end-to-end scene with its host embedding."""
import functools

import numpy as np

from tests.regions_cases import pattern

E2E = dict(rows=61, cols=47, K=9, G=3, step=4, shape=(103, 11, 11, 103, 9), channels=5, seed=1, param_seed=61)


def hub_map(rows, cols):
    """one-pixel background lines (region 0) around 2 x 2 cells (regions 1 ..): the background touches every cell with the
    same boundary length wherever the cell is whole, so truncation and ties to the smaller id decide its list.  (ids, M)"""
    yy, xx = np.divmod(np.arange(rows * cols), cols)
    ncx = -(-cols // 3)
    cell = (yy // 3) * ncx + xx // 3 + 1
    ids = np.where((yy % 3 == 0) | (xx % 3 == 0), 0, cell)
    return ids.astype(np.int32), int(-(-rows // 3) * ncx + 1)


@functools.lru_cache(maxsize=None)
def region_map(name, rows, cols):
    """(ids int32 [n], M) of a named map"""
    from cmlpl_amd.regions import cc_label_host
    n = rows * cols
    if name == "pixels":                                         # every interior region has 4 neighbours of length 1
        ids, M = np.arange(n, dtype=np.int32), n
    elif name == "one":
        ids, M = np.zeros(n, np.int32), 1
    elif name == "hub":
        ids, M = hub_map(rows, cols)
    elif name in ("components", "smoothed_components"):
        cc = cc_label_host(pattern("random9" if name == "components" else "smoothed", rows, cols, 4), rows, cols, 4)
        ids, M = cc["id"], max(1, cc["M"])
    elif name == "past_M":                                       # values 5 .. 8 are void
        ids, M = pattern("random9", rows, cols, 5), 5
    elif name == "empty":                                        # two regions in three stay empty
        ids, M = pattern("random9", rows, cols, 6) * 3, 30
    elif name == "voids":
        ids, M = pattern("voids", rows, cols, 7), 2
    elif name == "constant":
        ids, M = pattern("constant", rows, cols), 8
    else:                                                        # stripes_h, stripes_v, spiral, comb, checker
        ids, M = pattern(name, rows, cols), 4
    ids = np.ascontiguousarray(ids, np.int32)
    ids.setflags(write=False)
    return ids, int(M)


def embed_host(params, spectra):
    """the spectral embedding on the host: l2norm(relu(W x + b)) in fp32 (a NaN row where nothing is positive)"""
    W, b = (np.asarray(params[k], np.float32) for k in ("feat_spe.weight", "feat_spe.bias"))
    y = np.maximum(np.asarray(spectra, np.float32) @ W.T + b, np.float32(0))
    with np.errstate(all="ignore"):
        return (y / np.sqrt((y * y).sum(1, keepdims=True))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def e2e_case():
    """the end-to-end scene: dict(p [n, K], cube [rows, cols, C], Y, spectra [n, bands], params: the closed-form parameters
    of the member network, shape).  7-pixel regions of a seeded class each (tests/test_smooth_host.case); a pixel's spectrum
    is its class's prototype + 0.3 N(0,1)."""
    from oracle import cmlpl_oracle as O
    from tests.test_smooth_host import case
    c = E2E
    p, cube, Y = case(c["rows"], c["cols"], c["K"], c["G"], c["seed"], channels=c["channels"])
    rng = np.random.default_rng(17)
    proto = rng.standard_normal((c["K"], c["shape"][3])).astype(np.float32)
    spectra = (proto[Y] + 0.3 * rng.standard_normal((len(Y), c["shape"][3]))).astype(np.float32)
    params = O.closed_form_params(O.NetShape(*c["shape"]), c["param_seed"])
    for a in (p, cube, spectra):
        a.setflags(write=False)
    return dict(p=p, cube=cube, Y=Y, spectra=spectra, params=params, shape=c["shape"])
