"""GPU: the CUBE-FED training step (ABI 6: cmlpl_batch.d_cube / d_lab_pix / d_unl_pix).  The patch rows of a batch are
gathered from the resident scene cube inside the step -- no [rows][C][H][W] window tensor exists -- and everything the
step computes must be BIT-equal to the split-fed step on `extract_patches(cube, pix)`: the gather is a pure copy and the
noise counters do not depend on where a row came from.  The forward of the cube-fed step runs on the augmented rows as
plain rows; its staging puts the same values into the same LDS places as the raw-row route, so no downstream quantity
differs and the whole step is held to tolerance 0 directly (augmented rows included).
The rows themselves are held to the ORACLE's cut, over the gather's whole envelope, in tests/test_gpu_window_envelope.py."""
import ctypes as C

import pytest
import torch

from cmlpl_amd import HyperParams, NetShape, TrainEngine, _lib
from cmlpl_amd.patches import extract_patches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"B2": (103, 11, 11, 103, 9), "B5": (48, 15, 15, 48, 20), "P": (60, 20, 20, 103, 9)}


def _pixels(rows, cols, w, n, g):
    """n scene pixels: the four corners, one pixel on each margin closer than w/2 to the edge (and to no other edge),
    one interior pixel -- in the FIRST nine entries -- then seeded random ones"""
    hw = w // 2
    rm, cm = rows // 2, cols // 2
    rc = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1),
          (1, cm), (rows - 2, cm), (rm, 1), (rm, cols - 2), (rm, cm)]
    pix = [r * cols + c for r, c in rc] + torch.randint(0, rows * cols, (n - len(rc),), generator=g).tolist()
    pix = torch.tensor(pix, dtype=torch.int64)
    r, c = pix // cols, pix % cols
    near_r, near_c = (r < hw) | (r >= rows - hw), (c < hw) | (c >= cols - hw)
    for corner in (0, cols - 1, (rows - 1) * cols, rows * cols - 1):
        assert (pix[:9] == corner).any()
    assert ((r[:9] < hw) & ~near_c[:9]).any() and ((r[:9] >= rows - hw) & ~near_c[:9]).any()      # top / bottom margin
    assert ((c[:9] < hw) & ~near_r[:9]).any() and ((c[:9] >= cols - hw) & ~near_r[:9]).any()      # left / right margin
    assert (~near_r[:9] & ~near_c[:9]).any()                                                       # interior
    return pix


def _scene(shape, n_lab, n_unl, seed):
    Cc, H, W, bands, K = shape
    rows, cols = H + 9, W + 7                       # at least the window on each side, small enough to run in seconds
    g = torch.Generator().manual_seed(seed)
    cube = torch.randn(rows, cols, Cc, generator=g)
    lab_pix, unl_pix = _pixels(rows, cols, H, n_lab, g), _pixels(rows, cols, H, n_unl, g)
    X = torch.randn(n_lab, bands, generator=g)
    Y = torch.randint(0, K, (n_lab,), generator=g)
    Xu = torch.randn(n_unl, bands, generator=g)
    return [t.to(DEV).contiguous() for t in (cube, lab_pix, unl_pix, X, Y, Xu)]


def _engine(shape, bt, btu, hist_rows=8):
    eng = TrainEngine(NetShape(*shape), bt, btu, HyperParams(), device=DEV, seed=1088, hist_rows=hist_rows)
    eng.init_params_default(1088)
    return eng


def _state(eng):
    return [eng.params.clone(), eng.m.clone(), eng.v.clone(), eng.bank_feats.clone(), eng.bank_probs.clone(),
            eng.scalar_hist.clone(), eng.grads.clone()]


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: state tensor {i} differs, max |d| = {(x - y).abs().max().item():.3e}"


def _explicit(shape, bt, btu, g):
    Cc, H, W, bands, K = shape
    n, cls_in = bt + btu, NetShape(*shape).cls_in
    shp = [(bt, Cc, H, W), (bt, bands)] * 2 + [(btu, Cc, H, W), (btu, bands)] * 2
    noise = [torch.randn(*s, generator=g).to(DEV) for s in shp]
    keep = 1.0 - HyperParams().dropout
    dm = ((torch.rand(2, n, cls_in, generator=g) < keep).float() / keep).to(DEV).contiguous()
    return noise, dm


@pytest.mark.parametrize("indexed", [False, True], ids=["rows", "by-index"])
@pytest.mark.parametrize("explicit", [False, True], ids=["in-kernel-noise", "noise8+dropmask"])
@pytest.mark.parametrize("name,bt,btu", [("B2", 24, 40), ("P", 16, 16), ("B5", 16, 48)])
def test_cube_fed_step_is_bit_identical_to_the_split_fed_step(name, bt, btu, explicit, indexed):
    shape = SHAPES[name]
    n_lab, n_unl = (3 * bt, 3 * btu) if indexed else (bt, btu)
    cube, lab_pix, unl_pix, X, Y, Xu = _scene(shape, n_lab, n_unl, 7)
    XP, XPu = extract_patches(cube, lab_pix, shape[1]), extract_patches(cube, unl_pix, shape[1])
    g = torch.Generator().manual_seed(3)
    ea, eb = _engine(shape, bt, btu), _engine(shape, bt, btu)
    steps = 4                                                   # step 0 stops at the gradients, then k = 3 updates
    for s in range(steps):
        kw = {}
        if indexed:
            # step 0 takes the first bt / btu split rows (the corner / margin / interior pixels), shuffled; then any rows
            li = torch.randperm(bt if s == 0 else n_lab, generator=g)[:bt].to(DEV)
            ui = torch.randperm(btu if s == 0 else n_unl, generator=g)[:btu].to(DEV)
            kw.update(lab_idx=li, unl_idx=ui)
        if explicit:
            kw["noise"], kw["dropmask"] = _explicit(shape, bt, btu, g)
        kw["apply_update"] = s > 0
        ea.step(XP, X, Y, XPu, Xu, 1, s, **kw)
        eb.step(None, X, Y, None, Xu, 1, s, cube=cube, lab_pix=lab_pix, unl_pix=unl_pix, **kw)
        xa, xb = ea.debug_region("xn"), eb.debug_region("xn")
        assert torch.equal(xa, xb), f"{name} step {s}: augmented rows differ, max |d| = {(xa - xb).abs().max().item():.3e}"
        (la, fa), (lb, fb) = ea.outputs(), eb.outputs()
        assert torch.equal(la, lb) and torch.equal(fa, fb), f"{name} step {s}: logits / features differ"
        _same(_state(ea), _state(eb), f"{name} step {s}")       # (step 0: all 20 gradient tensors, nothing updated)
    assert ea.ptr == eb.ptr and ea.adam_t == eb.adam_t == steps - 1
    wa, wb = ea.loss_window(steps), eb.loss_window(steps)
    assert (wa == wb).all() and torch.isfinite(eb.scalar_hist[:steps]).all()


@pytest.mark.parametrize("name,bt,btu", [("B2", 24, 40), ("P", 16, 16)])
def test_cube_fed_graph_replay_is_bit_identical_to_cube_fed_eager(name, bt, btu):
    """one programmed epoch (4 full batches of the splits, crossing the smoothing gate of train.py:212) replayed from the
    captured cube-fed step against the same steps eager"""
    shape = SHAPES[name]
    cube, lab_pix, unl_pix, X, Y, Xu = _scene(shape, 4 * bt + 5, 4 * btu + 3, 11)
    g = torch.Generator().manual_seed(5)
    lab_perm = torch.randperm(X.shape[0], generator=g).to(DEV)
    unl_perm = torch.randperm(Xu.shape[0], generator=g).to(DEV)
    sched = [(0, 15), (0, 16), (0, 17), (0, 18), (0, 19)]
    offs = [(k % 4) * bt for k in range(len(sched))], [(k % 4) * btu for k in range(len(sched))]
    src = dict(cube=cube, lab_pix=lab_pix, unl_pix=unl_pix)
    ea, eb = _engine(shape, bt, btu, 16), _engine(shape, bt, btu, 16)
    for k, (ep, bi) in enumerate(sched):
        ea.step(None, X, Y, None, Xu, ep, bi, lab_idx=lab_perm[offs[0][k]:offs[0][k] + bt],
                unl_idx=unl_perm[offs[1][k]:offs[1][k] + btu], **src)
    ep, bi = sched[0]
    eb.step(None, X, Y, None, Xu, ep, bi, lab_idx=lab_perm[:bt], unl_idx=unl_perm[:btu], **src)
    graph = eb.capture(None, X, Y, None, Xu, lab_perm, unl_perm, bt, btu, capacity=16, **src)
    graph.program([(e, b, offs[0][k], offs[1][k]) for k, (e, b) in enumerate(sched)][1:])
    for _ in range(len(sched) - 1):
        graph.launch()
    torch.cuda.synchronize()
    assert ea.ptr == eb.ptr and ea.adam_t == eb.adam_t and ea.step_count == eb.step_count
    _same(_state(ea), _state(eb), f"{name} after {len(sched)} steps")
    assert torch.isfinite(eb.scalar_hist[:len(sched)]).all()
    graph.close()


def test_cube_fed_arguments_are_checked_on_the_host_and_in_the_library():
    shape = SHAPES["B2"]
    cube, lab_pix, unl_pix, X, Y, Xu = _scene(shape, 16, 16, 1)
    XP = extract_patches(cube, lab_pix, 11)
    eng = _engine(shape, 16, 16)
    src = dict(cube=cube, lab_pix=lab_pix, unl_pix=unl_pix)
    with pytest.raises(ValueError):
        eng.step(XP, X, Y, None, Xu, 0, 0, **src)                                    # windows AND the cube
    with pytest.raises(ValueError):
        eng.step(None, X, Y, None, Xu, 0, 0, cube=cube, lab_pix=lab_pix)             # a pixel list missing
    with pytest.raises(ValueError):
        eng.step(None, X, Y, None, Xu, 0, 0, cube=cube[:, :, :60].contiguous(), lab_pix=lab_pix, unl_pix=unl_pix)   # C mismatch
    with pytest.raises(ValueError):
        eng.step(None, X, Y, None, Xu, 0, 0, cube=cube[:8].contiguous(), lab_pix=lab_pix % 8, unl_pix=unl_pix % 8)  # scene < window
    bad = lab_pix.clone(); bad[3] = cube.shape[0] * cube.shape[1]
    with pytest.raises(ValueError):
        eng.step(None, X, Y, None, Xu, 0, 0, cube=cube, lab_pix=bad, unl_pix=unl_pix)                                # pixel out of range
    assert eng.step_count == 0
    eng.step(None, X, Y, None, Xu, 0, 0, **src)
    # the captured step refuses a malformed batch with the library's own error code, before any launch
    idx = torch.arange(16, device=DEV)
    io = _lib.StepIO()
    eng._fill_state(io)
    eng._fill_io(io, None, X, Y, None, Xu, idx, idx, 16, 16, cube, lab_pix, unl_pix)
    io.d_scalars, io.apply_update = eng.scalar_hist.data_ptr(), 1
    table, cursor = torch.zeros(4 * 64, dtype=torch.uint8, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    io.d_dyn_table, io.d_dyn_cursor = table.data_ptr(), cursor.data_ptr()
    io.d_xpl = XP.data_ptr()
    cap, handle = torch.cuda.Stream(device=DEV), C.c_void_p()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):
        rc = eng.lib.cmlpl_step_graph_create(C.byref(eng.cshape), C.byref(eng._chp), C.byref(io), C.c_void_p(cap.cuda_stream),
                                             C.byref(handle))
    torch.cuda.current_stream().wait_stream(cap)
    assert rc == -1 and not handle.value
    eng.step(None, X, Y, None, Xu, 0, 1, **src)                                      # the engine is still usable
    torch.cuda.synchronize()
    assert torch.isfinite(eng.scalar_hist).all()
