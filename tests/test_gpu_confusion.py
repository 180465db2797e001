"""GPU: the confusion-matrix kernel (cmlpl_confusion) against numpy.add.at on seeded vectors -- exact integer equality
(LDS and global INTEGER atomics: the order of the adds cannot matter), identical bytes on two runs."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu


def _confusion(pred, truth, K, cm=None, ignored=None):
    from cmlpl_amd import _lib
    lib = _lib.load()
    nets, n = pred.shape
    cm = torch.zeros(nets, K, K, dtype=torch.int64, device=DEV) if cm is None else cm
    ignored = torch.zeros(1, dtype=torch.int64, device=DEV) if ignored is None else ignored
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check("cmlpl_confusion", lib.cmlpl_confusion(pred.data_ptr(), nets, truth.data_ptr(), n, K, cm.data_ptr(),
                                                      ignored.data_ptr(), st))
    return cm, ignored


def _want(pred, truth, K):
    cm = np.zeros((pred.shape[0], K, K), dtype=np.int64)
    ok = (truth >= 0) & (truth < K)
    for k in range(pred.shape[0]):
        np.add.at(cm[k], (truth[ok], pred[k][ok]), 1)
    return cm, int((~ok).sum())


@pytest.mark.parametrize("n", [1, 1000, 42776])
@pytest.mark.parametrize("K", [1, 9, 20, 64])
@pytest.mark.parametrize("nets", [1, 2])
def test_confusion_equals_numpy(n, K, nets):
    rng = np.random.Generator(np.random.PCG64(1000 * K + n + nets))
    truth = rng.integers(0, K, n)
    pred = rng.integers(0, K, (nets, n))
    want, _ = _want(pred, truth, K)
    t, p = torch.from_numpy(truth).to(DEV), torch.from_numpy(pred).to(DEV)
    cm, ign = _confusion(p, t, K)
    again, _ = _confusion(p, t, K)
    assert np.array_equal(cm.cpu().numpy(), want) and int(ign) == 0
    assert cm.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    assert int(cm.sum()) == nets * n


@pytest.mark.parametrize("K", [1, 9, 64])
def test_confusion_all_one_class(K):
    """every row on one cell: the worst contention of the LDS atomics"""
    n = 42776
    truth = torch.full((n,), K - 1, dtype=torch.int64, device=DEV)
    pred = torch.full((2, n), K // 2, dtype=torch.int64, device=DEV)
    cm, ign = _confusion(pred, truth, K)
    want = np.zeros((2, K, K), dtype=np.int64)
    want[:, K - 1, K // 2] = n
    assert np.array_equal(cm.cpu().numpy(), want) and int(ign) == 0


def test_confusion_ignores_out_of_range_truths_and_accumulates():
    K, n = 9, 10007
    rng = np.random.Generator(np.random.PCG64(5))
    truth = rng.integers(-2, K + 2, n)                     # -2, -1, K, K + 1: unlabelled
    pred = rng.integers(0, K, (2, n))
    want, skipped = _want(pred, truth, K)
    assert skipped > 0
    t, p = torch.from_numpy(truth).to(DEV), torch.from_numpy(pred).to(DEV)
    cm, ign = _confusion(p, t, K)
    assert np.array_equal(cm.cpu().numpy(), want) and int(ign) == skipped
    # a second list added into the same matrix and counter (chunks, ranks)
    truth2 = rng.integers(-1, K, 777)
    pred2 = rng.integers(0, K, (2, 777))
    want2, skipped2 = _want(pred2, truth2, K)
    _confusion(torch.from_numpy(pred2).to(DEV), torch.from_numpy(truth2).to(DEV), K, cm, ign)
    assert np.array_equal(cm.cpu().numpy(), want + want2) and int(ign) == skipped + skipped2
    # the two halves of a list add up to the whole list's matrix
    h = n // 2
    a, ia = _confusion(p[:, :h].contiguous(), t[:h].contiguous(), K)
    _confusion(p[:, h:].contiguous(), t[h:].contiguous(), K, a, ia)
    assert np.array_equal(a.cpu().numpy(), want) and int(ia) == skipped
