"""GPU: the scene built on the device (cmlpl_scene_gram / cmlpl_scene_project through cmlpl_amd.scene) against the
REFERENCE sample_generation.py (tests/golden/patches_samplegen_ref.npz) and an fp64 numpy restatement, and the drop-in
sample_generation.py + train.py end to end without XP.npy."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.samplegen_util import CASES, load_case, ulp_report, write_mats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated(raw, n_pc):
    """fp64 numpy restatement of featureNormalize(PCANorm(X, n_PC), 1) and featureNormalize(X, 1)"""
    X = raw.reshape(-1, raw.shape[-1]).astype(np.float64)
    Xc = X - X.mean(0)
    U = np.linalg.svd(np.cov(Xc.T))[0]
    P = Xc @ U[:, :n_pc]
    return ((P - P.mean(0)) / P.std(0)).reshape(raw.shape[0], raw.shape[1], n_pc), Xc / Xc.std(0)


@pytest.mark.parametrize("c", CASES)
def test_cube_spectra_and_windows_match_the_reference(c):
    from cmlpl_amd.patches import extract_patches
    from cmlpl_amd.scene import build_scene
    d = load_case(c)
    cube, spectra = build_scene(d["raw"], d["n_PC"], DEV)
    assert cube.dtype == torch.float32 and tuple(cube.shape) == d["cube"].shape
    assert spectra.dtype == torch.float64 and tuple(spectra.shape) == (cube.shape[0] * cube.shape[1], d["raw"].shape[2])
    ulp_report(f"{c} cube", cube.cpu().numpy(), d["cube"].astype(np.float32))
    spec = spectra.cpu().numpy()
    want = d["X"] if d["X"].dtype == np.float64 else restated(d["raw"], d["n_PC"])[1]
    rel = np.max(np.abs(spec - want)) / np.max(np.abs(want))
    print(f"{c} spectra: max rel {rel:.2e}")
    assert rel <= 1e-12
    if d["X"].dtype == np.float32:       # the reference's own float32 featureNormalize (its float32 band means are
        assert np.max(np.abs(spec - d["X"])) <= 2e-4 * np.max(np.abs(want))      # summed row by row: ~1e-5 off)
    idx = torch.from_numpy(d["xp_idx"]).to(DEV)
    ulp_report(f"{c} XP rows", extract_patches(cube.contiguous(), idx, d["w"]).cpu().numpy(), d["xp"])


@pytest.mark.parametrize("c", CASES)
def test_gram_is_the_reference_covariance_and_keeps_its_signs(c):
    from cmlpl_amd import scene
    d = load_case(c)
    raw = d["raw"]
    n = raw.shape[0] * raw.shape[1]
    d_raw, code = scene._upload(raw, torch.device(DEV))
    ws = scene._workspace(n, raw.shape[2], d["n_PC"], torch.device(DEV))
    mean, gram = scene.scene_gram(d_raw, code, ws)
    X = raw.reshape(n, -1)
    Xn = X - np.mean(X, 0)                                  # the reference's PCANorm, hyper_tools.py:26-29
    cov = np.cov(Xn.T)
    got = gram.cpu().numpy() / (n - 1)
    scale = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    err = np.max(np.abs(got - cov) / scale)
    print(f"{c}: G/(N-1) vs np.cov max rel {err:.2e}")
    assert err <= 1e-12
    assert np.allclose(mean.cpu().numpy(), X.astype(np.float64).mean(0), rtol=1e-13, atol=0)
    U_ref = np.linalg.svd(cov)[0][:, :d["n_PC"]]
    U = scene.pca_basis(gram.cpu().numpy(), n, d["n_PC"])
    assert np.all(np.sum(U * U_ref, axis=0) > 0.999999)       # same vectors, same signs


def test_cube_is_deterministic_and_independent_of_the_dtype():
    from cmlpl_amd.scene import build_scene
    raw = load_case("a")["raw"]                              # uint16 values < 2^15
    cube0, spec0 = build_scene(raw, 6, DEV)
    c0, s0 = cube0.cpu().numpy(), spec0.cpu().numpy()
    for dt in (np.uint16, np.int16, np.float32, np.float64, np.int32):
        cube, spec = build_scene(raw.astype(dt), 6, DEV)
        assert np.array_equal(cube.cpu().numpy(), c0) and np.array_equal(spec.cpu().numpy(), s0), dt


def paviau_sized_scene(seed=3):
    """610 x 340 x 103 uint16 with a decaying spectrum: the first 60 eigenvalues about 6 % apart"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, cols, bands, k = 610, 340, 103, 64
    V = np.linalg.qr(rng.standard_normal((bands, bands)))[0][:, :k]
    A = rng.standard_normal((rows * cols, k)) * (1000.0 * 0.97 ** np.arange(k))
    x = 20000.0 + A @ V.T + 2.0 * rng.standard_normal((rows * cols, bands))
    return np.clip(np.rint(x), 0, 65535).astype(np.uint16).reshape(rows, cols, bands)


def test_paviau_sized_scene_against_fp64_numpy():
    """1 fp32 ulp, with an absolute floor of 1e-12 (in units of the component's std): two fp64 computations of this
    cube differ by about 1.5e-13 wherever they are summed in another order (numpy with 2048-pixel chunked sums against
    plain numpy: 1.5e-13, and one of the 12.4 M elements, of magnitude 5e-8, more than 1 ulp apart), so below ~1e-5 the
    ulp is finer than fp64 can decide"""
    from cmlpl_amd.scene import build_scene
    raw = paviau_sized_scene()
    cube, spectra = build_scene(raw, 60, DEV)
    want_cube, want_spec = restated(raw, 60)
    ulp_report("PaviaU-sized cube", cube.cpu().numpy(), want_cube.astype(np.float32), abs_floor=1e-12)
    spec = spectra.cpu().numpy()
    assert np.max(np.abs(spec - want_spec)) <= 1e-12 * np.max(np.abs(want_spec))


def test_loader_device_arrays_cut_the_host_windows():
    """HSIDataSet over a cube directory: device_arrays() (one extract_patches call) == the host cut, exactly"""
    import tempfile
    from hsi_loader import HSIDataSet
    from tests.test_samplegen import cube_dir
    d = load_case("b")
    with tempfile.TemporaryDirectory() as tmp:
        root = cube_dir(tmp, d)
        ds = HSIDataSet(3, "unlabel", max_iters=500, num_unlabel=200, root=root)
        XP, X, Y = ds.device_arrays(DEV)
        assert XP.is_cuda and tuple(XP.shape) == tuple(ds.XP.shape)
        host = np.stack([ds[i][0] for i in range(len(ds))])
        assert np.array_equal(XP.cpu().numpy(), host)


def test_sample_generation_then_train_without_xp(tmp_path):
    """the drop-in preprocessing on a tiny synthetic PaviaU, then train.py from that directory: no XP.npy anywhere, the
    evaluation straight from the cube (a window infer_supported takes)"""
    from cmlpl_amd import NetShape
    from cmlpl_amd.infer import infer_supported
    rng = np.random.Generator(np.random.PCG64(21))
    rows, cols, bands, K = 40, 36, 103, 9
    gt = (np.arange(rows * cols) // 160 % K + 1).astype(np.uint8).reshape(rows, cols)
    proto = rng.uniform(2000, 6000, size=(K, bands))
    raw = proto[gt.reshape(-1) - 1] + 150 * rng.standard_normal((rows * cols, bands))
    raw = np.clip(np.rint(raw), 0, 65535).astype(np.uint16).reshape(rows, cols, bands)
    out = write_mats(str(tmp_path), 1, raw, gt)
    w, n_pc = 8, 8
    assert infer_supported(NetShape(n_pc, w, w, bands, K))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sample_generation.py"), "--dataID", "1", "--num_label", "5",
                        "--w", str(w), "--n_PC", str(n_pc)], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    assert sorted(os.listdir(out)) == ["X.npy", "Y.npy", "cube.npy", "scene.json", "test_array.npy", "train_array.npy",
                                       "unlabel_array.npy"]
    from hsi_loader import HSIDataSet
    assert HSIDataSet(1, "wholeset", root=out + "/").cube_source(DEV, dataID=1) is not None
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--dataID", "1", "--num_epochs", "1",
                        "--num_unlabel", "256", "--labeled_batch_size", "64", "--unlabeled_batch_size", "64"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert "OA=" in r.stdout and "Kappa=" in r.stdout and "OA1=" in r.stdout
    assert not any("XP.npy" in f for _, _, fs in os.walk(tmp_path) for f in fs)
