"""CPU: flip / rotate windows (include/cmlpl.h, "THE DEFINITION OF A SPATIAL ELEMENT") restated in numpy -- the index
map of the eight elements, the element a training row takes (the hash of tests/test_noise_generator_math.py), the blocks
of a spatial ``TTA`` -- and what the C ABI, the Python wrappers and the two command lines refuse, without a device.
tests/test_gpu_spatial.py holds the kernels to ``spatial_index`` and ``training_elements``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_noise_generator_math import _ctr, noise_hash_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE = -1, -2
FAKE = 0x10000
STREAM_SYM = 0x600
MODES = {"none": 1, "flips": 4, "d4": 8}
ROT90 = 5                       # the element the header names as rot90(k=1)


# ------------------------------------------------------------------ the definition
def spatial_index(g, w):
    """src [w * w]: output pixel p = i w + j of element g shows window pixel src[p] = i' w + j'"""
    i, j = np.divmod(np.arange(w * w), w)
    a, b = (j, i) if g & 4 else (i, j)
    si = w - 1 - a if g & 2 else a
    sj = w - 1 - b if g & 1 else b
    return si * w + sj


def apply_element(win, g):
    """element g of windows [..., w, w]"""
    w = win.shape[-1]
    return win.reshape(*win.shape[:-2], w * w)[..., spatial_index(g, w)].reshape(win.shape)


def training_elements(seed, step, samples, mode):
    """the element of the rows with global sample indices ``samples`` at step counter ``step``: the TOP three bits of the hash
    word (its low bits are one value for 256 consecutive samples -- counts of 256 .. 1280 per element over 4,096 samples,
    where the test below allows 512 +- 106 -- because noise_ctr leaves the counter's low 24 bits zero)"""
    samples = np.asarray(samples, np.uint64)
    words = noise_hash_words(seed, step, STREAM_SYM, _ctr(samples, np.zeros(len(samples), np.uint64)))      # noise_ctr(gs, 0)
    return ((words[0] >> np.uint64(29)) & np.uint64(MODES[mode] - 1)).astype(np.int64)


@pytest.mark.parametrize("w", [4, 5])
def test_the_eight_elements_are_the_dihedral_group(w):
    win = np.random.default_rng(w).standard_normal((3, w, w)).astype(np.float32)      # asymmetric data
    idx = [spatial_index(g, w) for g in range(8)]
    for g in range(8):
        assert sorted(idx[g]) == list(range(w * w))                                   # a permutation of the same pixels
    assert len({tuple(i) for i in idx}) == 8                                          # all distinct
    out = [apply_element(win, g) for g in range(8)]
    assert np.array_equal(out[0], win)
    assert np.array_equal(out[1], np.flip(win, -1)) and np.array_equal(out[2], np.flip(win, -2))
    assert np.array_equal(out[3], np.rot90(win, 2, axes=(-2, -1)))
    assert np.array_equal(out[4], np.swapaxes(win, -1, -2))
    assert np.array_equal(out[ROT90], np.rot90(win, 1, axes=(-2, -1)))
    assert np.array_equal(out[6], np.rot90(win, 3, axes=(-2, -1)))
    assert np.array_equal(out[7], np.flip(np.flip(np.swapaxes(win, -1, -2), -1), -2))
    # closed under composition, and g in 0..3 is a subgroup (the reference's flip)
    table = np.full((8, 8), -1)
    for g in range(8):
        for h in range(8):
            both = apply_element(out[g], h)
            hit = [k for k in range(8) if np.array_equal(both, out[k])]
            assert len(hit) == 1, (g, h)
            table[g, h] = hit[0]
    assert all(sorted(row) == list(range(8)) for row in table)
    assert set(table[:4, :4].ravel()) == {0, 1, 2, 3}


def test_the_header_states_the_definition():
    text = open(os.path.join(ROOT, "include", "cmlpl.h")).read()
    assert "THE DEFINITION OF A SPATIAL ELEMENT" in text and "THE DEFINITION OF A VIEW" in text
    assert re.search(r"#define\s+CMLPL_ABI_VERSION\s+6\b", text)
    assert re.search(r"CMLPL_STREAM_SYM\s*=\s*0x600\b", text)
    assert re.search(r"CMLPL_SYM_NONE\s*=\s*0,\s*CMLPL_SYM_FLIPS\s*=\s*1,\s*CMLPL_SYM_D4\s*=\s*2", text)
    flat = " ".join(text.split())
    assert "g = %d the quarter turn rot90(k=1)" % ROT90 in flat
    for piece in ("(a, b) = (g & 4) ? (j, i) : (i, j)", "i' = (g & 2) ? w - 1 - a : a", "j' = (g & 1) ? w - 1 - b : b",
                  "g = (noise_hash(seed, step, CMLPL_STREAM_SYM, noise_ctr(gs, 0)).x >> 29) & (S - 1)"):
        assert piece in flat, piece


def test_the_training_element_is_uniform_and_flips_stay_below_four():
    gs = np.arange(4096)
    g = training_elements(1088, 3, gs, "d4")
    counts = np.bincount(g, minlength=8)
    assert counts.sum() == 4096 and len(counts) == 8
    assert (np.abs(counts - 512) <= 5 * np.sqrt(448)).all(), counts                   # binomial(4096, 1/8): variance 448
    f = training_elements(1088, 3, gs, "flips")
    assert f.max() <= 3 and len(set(f.tolist())) == 4 and np.array_equal(f, g & 3)
    assert (training_elements(1088, 3, gs, "none") == 0).all()
    assert not np.array_equal(g, training_elements(1088, 4, gs, "d4"))                # the step counts
    assert not np.array_equal(g, training_elements(1089, 3, gs, "d4"))                # and the seed


# ------------------------------------------------------------------ the C ABI
def _lib_loaded():
    from cmlpl_amd import _lib, build_ext
    if build_ext.needs_build():
        build_ext.build(verbose=False)
    return _lib, _lib.load()


NEW = ("cmlpl_infer_cube_tta_sym", "cmlpl_infer_pixels_tta_sym", "cmlpl_tta_patches_sym")
# sizeof and the field offsets as they are on the parent commit
STEP_IO = (296, {'d_xpl': 0, 'd_xl': 8, 'd_labels': 16, 'd_xpu': 24, 'd_xu': 32, 'noise8': 40, 'd_dropmask': 48, 'd_params': 56,
                 'd_m': 64, 'd_v': 72, 'd_grads': 80, 'd_packed': 88, 'banks': 96, 'd_scalars': 144, 'd_logits': 152, 'd_feat': 160,
                 'd_workspace': 168, 'workspace_bytes': 176, 'bt': 184, 'btu': 188, 'smooth': 192, 'adap_mask': 196, 'adam_t': 200,
                 'seed': 208, 'step': 216, 'apply_update': 224, 'reserved': 228, 'd_lab_idx': 232, 'd_unl_idx': 240,
                 'd_dyn_table': 248, 'd_dyn_cursor': 256, 'd_cube': 264, 'cube_rows': 272, 'cube_cols': 276, 'd_lab_pix': 280,
                 'd_unl_pix': 288})
BATCH = (104, {'d_xpl': 0, 'd_xl': 8, 'd_xpu': 16, 'd_xu': 24, 'd_labels': 32, 'noise8': 40, 'bt': 48, 'btu': 52, 'd_lab_idx': 56,
               'd_unl_idx': 64, 'd_cube': 72, 'cube_rows': 80, 'cube_cols': 84, 'd_lab_pix': 88, 'd_unl_pix': 96})
DYN = (64, {'step': 0, 'adam_t': 8, 'lab_off': 16, 'unl_off': 24, 'ptr': 32, 'smooth': 40, 'adap_mask': 44, 'hist_row': 48,
            'adam_step_size': 52, 'adam_bc2_sqrt': 56, 'reserved': 60})


def test_exports_resolve_and_no_record_moved():
    _lib, lib = _lib_loaded()
    for s in NEW:
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert _lib.ABI_VERSION == 6 and lib.cmlpl_abi_version() == 6
    for name, (size, offsets) in (("StepIO", STEP_IO), ("Batch", BATCH), ("Dyn", DYN)):
        t = getattr(_lib, name)
        assert C.sizeof(t) == size, name
        assert {f[0]: getattr(t, f[0]).offset for f in t._fields_} == offsets, name
    for old, new in (("cmlpl_infer_cube_tta", NEW[0]), ("cmlpl_infer_pixels_tta", NEW[1]), ("cmlpl_tta_patches", NEW[2])):
        assert list(getattr(lib, new).argtypes) == list(getattr(lib, old).argtypes) + [C.c_uint32]
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cmlpl.h")).read(), flags=re.S)
    for old, new in (("cmlpl_infer_cube_tta", NEW[0]), ("cmlpl_infer_pixels_tta", NEW[1]), ("cmlpl_tta_patches", NEW[2])):
        proto = lambda name: [" ".join(p.split()[:-1]) for p in re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code).group(1).split(",")]
        assert proto(new) == proto(old) + ["uint32_t"], new
    assert _lib.SPATIAL == {"none": 0, "flips": 1, "d4": 2} and [_lib.spatial_elements(m) for m in MODES] == list(MODES.values())
    b2 = _lib.Shape(103, 11, 11, 103, 9)                                     # (no workspace of their own)
    assert lib.cmlpl_infer_tta_workspace_bytes(C.byref(b2), 100) > 0


def _fused(lib, which, sym, sigma=0.5, shape=(103, 11, 11, 103, 9)):
    from cmlpl_amd import _lib
    cs = _lib.Shape(*shape)
    if which == "cube":
        return lib.cmlpl_infer_cube_tta_sym(C.byref(cs), FAKE, FAKE, FAKE, 24, 20, FAKE, 0, 16, FAKE, None, FAKE, 1 << 30, None,
                                            sigma, 1088, 0, sym)
    return lib.cmlpl_infer_pixels_tta_sym(C.byref(cs), 1, FAKE, 1 << 24, FAKE, 1 << 24, FAKE, 24, 20, FAKE, None, FAKE, 16, FAKE,
                                          None, FAKE, 1 << 30, None, sigma, 1088, 0, sym)


def test_the_view_entry_points_refuse_a_bad_element_before_any_launch():
    """every call here is refused on the host: had one launched, it would have failed another way without a device"""
    _, lib = _lib_loaded()
    for which in ("cube", "pixels"):
        for sym in (8, 9, 255, 2 ** 31):
            assert _fused(lib, which, sym) == E_ARG and _fused(lib, which, sym, sigma=0.0) == E_ARG, (which, sym)
        for sym in (4, 5, 6, 7):
            assert _fused(lib, which, sym, shape=(103, 11, 13, 103, 9)) == E_SHAPE, (which, sym)
        assert _fused(lib, which, 3, sigma=-1.0) == E_ARG                         # what the functions without _sym refuse
    f = lambda sym, **k: lib.cmlpl_tta_patches_sym(*[k.get(a, d) for a, d in (
        ("cube", FAKE), ("rows", 24), ("cols", 20), ("C", 103), ("w", 11), ("pix", FAKE), ("n", 8), ("out", FAKE), ("spectra", FAKE),
        ("spec_row", None), ("bands", 103), ("spectra_out", FAKE), ("sigma", 0.5), ("seed", 1088), ("view", 0), ("stream", None))], sym)
    assert f(8) == E_ARG and f(2 ** 32 - 1) == E_ARG
    assert f(5, pix=None) == E_ARG and f(5, w=50) == E_SHAPE and f(5, n=0) == E_ARG


def _step(lib, reserved, cube=FAKE):
    from cmlpl_amd import _lib
    io = _lib.StepIO()
    for name in ("d_xl", "d_labels", "d_xu", "d_params", "d_m", "d_v", "d_grads", "d_packed", "d_scalars", "d_logits", "d_feat",
                 "d_workspace"):
        setattr(io, name, FAKE)
    io.bt = io.btu = 16
    io.workspace_bytes = 1024                                               # too small: a call that passes the checks ends here
    io.apply_update, io.reserved = 1, reserved
    if cube:
        io.d_cube, io.d_lab_pix, io.d_unl_pix, io.cube_rows, io.cube_cols = cube, FAKE, FAKE, 24, 20
    else:
        io.d_xpl = io.d_xpu = FAKE
    io.banks.Q = 320
    cs, hp = _lib.Shape(103, 11, 11, 103, 9), _lib.HParams()
    return lib.cmlpl_train_step(C.byref(cs), C.byref(hp), C.byref(io), None)


def test_the_step_refuses_bad_mode_bits_before_any_launch():
    _, lib = _lib_loaded()
    E_WORKSPACE = -3
    for method in (0, 1):
        for mode in (0, 1, 2):
            assert _step(lib, method | (mode << 8)) == E_WORKSPACE, (method, mode)          # legal: refused later, for its workspace
        assert _step(lib, method | (3 << 8)) == E_ARG
        assert _step(lib, method | (1 << 10)) == E_ARG and _step(lib, method | (1 << 8) | (1 << 16)) == E_ARG
        assert _step(lib, method | (1 << 8), cube=None) == E_ARG and _step(lib, method | (2 << 8), cube=None) == E_ARG
        assert _step(lib, method, cube=None) == E_WORKSPACE
    assert _step(lib, 2) == E_ARG and _step(lib, 2 | (1 << 8)) == E_ARG and _step(lib, -1) == E_ARG


# ------------------------------------------------------------------ the Python wrappers
def test_tta_blocks_over_the_three_modes():
    from cmlpl_amd.tta import TTA, _check_blocks, _key
    assert TTA(3, 0.5).spatial == "none"
    assert TTA(3, 0.5).blocks() == [None, 0, 1, 2] and TTA(3, 0.5, clean=False).blocks() == [0, 1, 2]
    assert TTA(3, 0.5).pairs() == [(None, 0), (0, 0), (1, 0), (2, 0)]
    assert TTA(5, 0.5, spatial="flips").blocks() == [(None, 0), (0, 1), (1, 2), (2, 3), (3, 0), (4, 1)]
    assert TTA(5, 0.5, clean=False, spatial="flips").blocks() == [(0, 0), (1, 1), (2, 2), (3, 3), (4, 0)]
    assert TTA(9, 0.5, spatial="d4").blocks() == [(None, 0)] + [(t, (t + 1) % 8) for t in range(9)]
    assert TTA(9, 0.5, clean=False, spatial="d4").blocks() == [(t, t % 8) for t in range(9)]
    orbit = TTA(7, 0.0, clean=True, spatial="d4")                            # sigma 0 is legal: pure geometry
    assert sorted(g for _, g in orbit.blocks()) == list(range(8))
    assert sorted(g for _, g in TTA(3, 0.0, spatial="flips").blocks()) == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="spatial"):
        TTA(3, 0.5, spatial="rot").blocks()
    with pytest.raises(ValueError, match="TTA"):
        TTA(-1, 0.5, spatial="d4").blocks()
    assert len(_check_blocks(TTA(15, 0.5, spatial="d4"), 4)) == 16
    with pytest.raises(ValueError, match="64"):
        _check_blocks(TTA(16, 0.5, spatial="d4"), 4)
    # a block's key: the clean block is sigma 0 under the identity; a pair, or g beside t
    val = lambda key: tuple(v.value for v in key)
    assert val(_key(orbit, None)) == (0.0, 1088, 0, 0) and val(_key(TTA(3, 0.5), 2)) == (0.5, 1088, 2, 0)
    assert val(_key(TTA(3, 0.5, spatial="d4"), (2, 3))) == (0.5, 1088, 2, 3) == val(_key(TTA(3, 0.5), 2, 3))
    for bad in ((2, 8), (2, -1), (None, 1)):
        with pytest.raises(ValueError, match="spatial element"):
            _key(TTA(3, 0.5), bad)


def test_the_engines_refuse_what_they_cannot_take():
    from cmlpl_amd import NetShape, TrainEngine
    from cmlpl_amd.distributed import DistTrainEngine
    from cmlpl_amd.engine import StepGraph
    shape = NetShape(103, 11, 11, 103, 9)
    with pytest.raises(ValueError, match="spatial"):
        TrainEngine(shape, 16, 16, aug_spatial="rot90")                       # (before any device work)
    for mode in ("flips", "d4"):
        with pytest.raises(ValueError, match="sharded"):
            DistTrainEngine(shape, 16, 16, aug_spatial=mode)
    # a split-fed step of an engine with a mode: refused before anything is looked at (an engine without a device)
    eng = TrainEngine.__new__(TrainEngine)
    eng.aug_spatial, eng._graph, eng.shape = "d4", None, shape
    with pytest.raises(ValueError, match="cube-fed"):
        eng.step(object(), None, None, object(), None, 0, 0)
    import torch
    idx = torch.zeros(16, dtype=torch.int64)
    with pytest.raises(ValueError, match="cube-fed"):
        StepGraph(eng, object(), None, None, object(), None, idx, idx, 16, 16)
    eng.aug_spatial = "none"
    eng._refuse_split_fed()
    # the identity record: a key only when there is a mode, and a difference either way
    from cmlpl_amd import HyperParams
    from cmlpl_amd.checkpoint import identity_differences, make_identity
    ids = {m: make_identity(shape, HyperParams(), 16, 16, 320, "h", 6, aug_spatial=m) for m in MODES}
    assert ids["none"] == make_identity(shape, HyperParams(), 16, 16, 320, "h", 6) and "aug_spatial" not in ids["none"]
    assert ids["d4"]["aug_spatial"] == "d4"
    for a, b in (("none", "d4"), ("d4", "none"), ("flips", "d4")):
        assert any(d.startswith("aug_spatial") for d in identity_differences(ids[a], ids[b])), (a, b)
    assert identity_differences(ids["d4"], ids["d4"]) == []


# ------------------------------------------------------------------ the command lines
def test_the_parsers_take_the_flags_and_refuse_as_specified(monkeypatch):
    import predict
    import train
    p = train.build_parser()
    a = p.parse_args(["--synthetic", "B2"])
    assert a.aug_spatial == "none" and a.tta_spatial == "none"
    train.check_spatial_args(a)
    for mode in ("flips", "d4"):
        a = p.parse_args(["--synthetic", "B2", "--windows", "cube", "--aug_spatial", mode, "--tta", "--tta_spatial", mode])
        assert a.aug_spatial == mode and a.tta_spatial == mode
        train.check_spatial_args(a)
        with pytest.raises(SystemExit) as e:                                 # under the launcher: at once
            train.check_spatial_args(a, world=2)
        assert "--aug_spatial" in str(e.value) and "one GPU" in str(e.value)
        with pytest.raises(SystemExit) as e:
            train.check_spatial_args(p.parse_args(["--synthetic", "B2", "--aug_spatial", mode]))
        assert "--windows cube" in str(e.value)
        with pytest.raises(SystemExit) as e:
            train.check_spatial_args(p.parse_args(["--synthetic", "B2", "--tta_spatial", mode]))
        assert "--tta" in str(e.value)
    with pytest.raises(SystemExit):
        p.parse_args(["--synthetic", "B2", "--aug_spatial", "rot"])

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    import torch
    monkeypatch.setattr(torch.cuda, "set_device", boom)
    with pytest.raises(SystemExit):
        train.main(p.parse_args(["--synthetic", "B2", "--aug_spatial", "d4"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        train.main(p.parse_args(["--synthetic", "B2", "--windows", "cube", "--aug_spatial", "d4"]))
    monkeypatch.delenv("WORLD_SIZE")

    q = predict.build_parser()
    assert q.parse_args(["--ckpt", "x"]).tta_spatial == "none"
    predict.check_args(q.parse_args(["--ckpt", "x"]))
    for net in ("0", "1", "ema0", "ensemble", "ensemble_all"):
        a = q.parse_args(["--ckpt", "x", "--net", net, "--tta", "7", "--tta_noise", "0", "--tta_spatial", "d4", "--smooth", "2",
                          "--proba", "p.npy"])
        assert (a.tta, a.tta_noise, a.tta_spatial) == (7, 0.0, "d4")
        predict.check_args(a)
    with pytest.raises(SystemExit) as e:
        predict.check_args(q.parse_args(["--ckpt", "x", "--tta_spatial", "d4"]))
    assert "--tta_spatial" in str(e.value)
    with pytest.raises(SystemExit):
        predict.check_args(q.parse_args(["--ckpt", "x", "--net", "both", "--tta", "3", "--tta_spatial", "flips"]))
    from cmlpl_amd.tta import TTA
    assert train.tta_tag(TTA(3, 0.5)) == "_tta" and train.tta_tag(TTA(3, 0.5, spatial="flips")) == "_tta_flips"
    assert train.tta_tag(TTA(7, 0.0, spatial="d4")) == "_tta_d4"
    assert train.tta_timing(TTA(5, 0.5)) == 'tta inference time == %.3f s (%d networks x 5 views + the clean window, noise 0.5)'


def test_saved_args_and_run_record_carry_the_mode_only_when_there_is_one():
    import train
    from cmlpl_amd import HyperParams
    p = train.build_parser()
    a0 = p.parse_args(["--synthetic", "B2", "--windows", "cube"])
    a1 = p.parse_args(["--synthetic", "B2", "--windows", "cube", "--aug_spatial", "d4", "--tta", "--tta_spatial", "d4"])
    s0, s1 = train.saved_args(a0), train.saved_args(a1)
    assert "aug_spatial" not in s0 and "tta_spatial" not in s0
    assert s1["aug_spatial"] == "d4" and s1["tta_spatial"] == "d4"
    assert {k: v for k, v in s1.items() if k not in ("aug_spatial", "tta_spatial", "tta")} == s0
    r0, r1 = (train.run_record(a, HyperParams(), train.SYNTH["B2"], True) for a in (a0, a1))
    assert "aug_spatial" not in r0 and r1["aug_spatial"] == "d4"
    assert train.run_differences(r0, r1) and train.run_differences(r1, r0) and train.run_differences(r1, r1) == []
