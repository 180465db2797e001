"""CPU: the host side of validation.  ``cmlpl_amd.evaluate.metrics`` (OA / Kappa / per-class accuracy / AA from a
confusion matrix) against ``tools.hyper_tools.CalAccuracy`` on seeded label vectors -- both are fp64 arithmetic on the
same integer counts, hence rtol 1e-12 --, and ``tools.hyper_tools.test_acc``'s loader path against the answer of the
reference's own ``test_acc`` on the seeded case of tests/testacc_util.py (tests/golden/eval/testacc_ref.npz, recorded by
tests/golden/make_golden_testacc.py)."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL = 1e-12


def _matrix(truth, pred, K):
    cm = np.zeros((K, K), dtype=np.int64)
    np.add.at(cm, (truth, pred), 1)
    return cm


def _compare(truth, pred, K):
    from cmlpl_amd.evaluate import Evaluator, metrics
    from tools.hyper_tools import CalAccuracy
    OA, Kappa, prodA = CalAccuracy(pred, truth)
    for fn in (metrics, Evaluator.metrics):
        for cm in (_matrix(truth, pred, K), torch.from_numpy(_matrix(truth, pred, K))):
            oa, kappa, pa, aa = fn(cm)
            np.testing.assert_allclose(oa, OA, rtol=RTOL, atol=0)
            np.testing.assert_allclose(kappa, Kappa, rtol=RTOL, atol=1e-15)
            assert pa.shape == prodA.shape
            np.testing.assert_allclose(pa, prodA, rtol=RTOL, atol=0)
            np.testing.assert_allclose(aa, np.mean(prodA), rtol=RTOL, atol=0)


@pytest.mark.parametrize("K", list(range(1, 21)))
def test_metrics_equal_calaccuracy(K):
    rng = np.random.Generator(np.random.PCG64(100 + K))
    n = 5000
    truth = rng.integers(0, K, n)
    truth[:K] = np.arange(K)                               # every class occurs
    pred = np.where(rng.random(n) < 0.7, truth, rng.integers(0, K, n))
    _compare(truth, pred, K)
    _compare(truth, pred, 64)                              # the same counts in a wider matrix (the device's K)


@pytest.mark.parametrize("absent", ["middle", "last", "last_but_predicted"])
def test_metrics_with_an_absent_class(absent):
    """CalAccuracy sizes its matrix by max(label) + 1 and clips the predictions into it; a class without a sample has
    producer's accuracy 0 and still counts in the mean"""
    K = 9
    rng = np.random.Generator(np.random.PCG64(7))
    n = 3000
    gone = 4 if absent == "middle" else K - 1
    truth = rng.integers(0, K - 1, n)
    truth = np.where(truth >= gone, truth + 1, truth) if absent == "middle" else truth
    pred = np.where(rng.random(n) < 0.6, truth, rng.integers(0, K, n))
    if absent == "last":
        pred = np.minimum(pred, K - 2)
    assert gone not in truth and (absent != "last_but_predicted" or (pred == K - 1).any())
    _compare(truth, pred, K)


def test_test_acc_loader_path_matches_the_reference(capsys):
    from tests.testacc_util import EPOCH, NUM_CLASSES, PRINT_EVERY, case
    from tools.hyper_tools import test_acc
    ref = np.load(os.path.join(HERE, "golden", "eval", "testacc_ref.npz"))
    model, loader = case()
    torch_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self          # CPU run, as the generator's
    try:
        acc = test_acc(model, loader, EPOCH, NUM_CLASSES, print_per_batches=PRINT_EVERY)
    finally:
        torch.Tensor.cuda = torch_cuda
    printed = capsys.readouterr().out
    assert isinstance(acc, float)
    np.testing.assert_allclose(acc, float(ref["acc"][0]), rtol=RTOL, atol=0)
    assert printed == bytes(ref["printed"]).decode()
    import re
    got = [float(m) for m in re.findall(r"Accuracy of\s+\d+ : ([0-9.]+) %", printed)]
    np.testing.assert_allclose(got, ref["per_class_percent"], rtol=0, atol=0)
