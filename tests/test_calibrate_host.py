"""CPU: the calibration definitions restated in numpy (cmlpl_amd.calibrate: reliability_host, temper_host, nll_temps_host), the
``Reliability`` block's derived numbers, the candidate grid of ``fit_temperature`` and the drivers' refusals.  No device."""
import math

import numpy as np
import pytest

from cmlpl_amd import calibrate as cal
from cmlpl_amd.calibrate import FIX20, FIX24, REL_HEAD, Reliability, reliability_host, temper_host

NAN = float("nan")


def hand_block():
    """K = 3, B = 4 (a power of two: the edges k / B are exact); every probability is dyadic, so every sum is exact"""
    probs = np.array([[0.5, 0.5, 0.0],          # t 0: a tie, the first maximum wins: hit; conf 0.5 = 2 / 4 exactly: the UPPER bin 2
                      [NAN, 0.2, 0.3],          # t 1: a NaN row
                      [0.2, 0.3, 0.5],          # t -1: unknown truth
                      [0.0, 0.0, 1.0],          # t 2: conf == 1: the last bin
                      [0.75, 0.25, 0.0],        # t 2: a miss with p_t = 0: n_inf; conf 0.75 = 3 / 4: the upper bin 3
                      [0.25, 0.25, 0.5],        # t 3 == K: unknown truth
                      [0.125, 0.625, 0.25]],    # t 1: hit, conf 0.625: bin 2
                     np.float32)
    truth = np.array([0, 1, -1, 2, 2, 3, 1], np.int64)
    return probs, truth


def fix24(x):
    return int(np.rint(float(np.float32(x)) * FIX24))


def test_reliability_host_equals_the_block_worked_out_by_hand():
    probs, truth = hand_block()
    r = reliability_host(probs, truth, None, bins=4)
    assert r.counts.shape == (REL_HEAD + 12,)
    assert (r.items, r.known, r.ignored, r.nan, r.hits, r.n_inf, r.scored) == (7, 5, 2, 1, 3, 1, 4)
    assert r.sum_conf == int((0.5 + 1.0 + 0.75 + 0.625) * FIX24)
    assert r.sum_nll == fix24(-math.log(0.5)) + 0 + fix24(-math.log(0.625))
    assert r.sum_brier == int((0.5 + 0.0 + 1.625 + 0.21875) * FIX24)
    assert not r.counts[9:REL_HEAD].any()
    assert r.count.tolist() == [0, 0, 2, 2] and r.bin_hits.tolist() == [0, 0, 2, 1]
    assert r.conf_sum.tolist() == [0, 0, int(1.125 * FIX24), int(1.75 * FIX24)]
    assert r.nll == float("inf") and r.accuracy == 0.75 and r.mean_conf == 2.875 / 4 and r.brier == 2.34375 / 4
    assert r.ece == 0.5 * 0.4375 + 0.5 * 0.375 and r.mce == 0.4375
    # the same items through a row list with repeats, over a larger map
    big = np.concatenate([np.full((2, 3), 1 / 3, np.float32), probs[::-1]])
    rows = np.array([8, 7, 6, 5, 4, 3, 2], np.int64)
    assert reliability_host(big, truth, rows, bins=4) == r
    # halves add up to the whole
    assert reliability_host(probs[:3], truth[:3], None, 4) + reliability_host(probs, truth[3:], np.arange(3, 7), 4) == r
    # without the p_t = 0 row the NLL is finite
    keep = np.array([0, 1, 2, 3, 5, 6])
    r2 = reliability_host(probs, truth[keep], keep, 4)
    assert r2.n_inf == 0 and r2.nll == (fix24(-math.log(0.5)) + fix24(-math.log(0.625))) / FIX24 / 3


def test_bins_clamp_and_one_bin():
    probs = np.array([[1.5, 0.0], [-0.5, -1.0], [0.999, 0.001], [np.inf, 0.0]], np.float32)
    truth = np.zeros(4, np.int64)
    r = reliability_host(probs[:3], truth[:3], None, bins=8)
    assert r.count.tolist() == [1, 0, 0, 0, 0, 0, 0, 2]               # conf > 1 into the last bin, conf < 0 into the first
    assert reliability_host(probs[3:], truth[3:], None, bins=8).count.tolist() == [0] * 7 + [1]
    one = reliability_host(probs[:3], truth[:3], None, bins=1)
    assert one.count.tolist() == [3] and one.counts.size == REL_HEAD + 3
    with pytest.raises(ValueError):
        reliability_host(probs, truth, None, bins=1025)
    with pytest.raises(ValueError):
        Reliability(np.zeros(REL_HEAD + 4, np.int64))
    with pytest.raises(ValueError):
        Reliability.zeros(4) + Reliability.zeros(5)


def _scalar_numbers(r):
    """ece, mce, curve and risk-coverage from the block's words with python scalars"""
    B = r.bins
    w = [int(v) for v in r.counts]
    count, hits, csum = w[REL_HEAD:REL_HEAD + B], w[REL_HEAD + B:REL_HEAD + 2 * B], w[REL_HEAD + 2 * B:]
    scored = w[1] - w[3]
    ece, mce, curve = 0.0, None, []
    for b in range(B):
        if count[b] == 0:
            curve.append((0, NAN, NAN))
            continue
        acc, conf = hits[b] / count[b], csum[b] / FIX24 / count[b]
        curve.append((count[b], acc, conf))
        ece += count[b] / scored * abs(acc - conf)
        mce = abs(acc - conf) if mce is None else max(mce, abs(acc - conf))
    rc, n, h = [], 0, 0
    for b in range(B - 1, -1, -1):
        n, h = n + count[b], h + hits[b]
        rc.append((n / scored, h / n if n else NAN))
    return ece, mce, curve, rc


@pytest.mark.parametrize("bins", [1, 15, 64, 1024])
def test_ece_mce_curve_and_risk_coverage_against_a_scalar_restatement(bins):
    rng = np.random.Generator(np.random.PCG64(bins))
    z = 3.0 * rng.standard_normal((500, 7))
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    truth = np.where(rng.random(500) < 0.7, p.argmax(axis=1), rng.integers(0, 7, 500)).astype(np.int64)
    truth[::50] = -1
    r = reliability_host(p, truth, None, bins)
    ece, mce, curve, rc = _scalar_numbers(r)
    assert r.ece == pytest.approx(ece, rel=1e-12) and r.mce == pytest.approx(mce, rel=1e-12)
    count, acc, conf = r.curve()
    cov, racc = r.risk_coverage()
    for b in range(bins):
        assert count[b] == curve[b][0]
        np.testing.assert_allclose([acc[b], conf[b]], curve[b][1:], rtol=1e-12, equal_nan=True)
        np.testing.assert_allclose([cov[b], racc[b]], rc[b], rtol=1e-12, equal_nan=True)
    assert cov[-1] == 1.0 and racc[-1] == pytest.approx(r.accuracy) and r.count.sum() == r.scored == 490
    assert r.line("_x", " (n)").startswith("Reliability_x: ECE=%.4f MCE=%.4f NLL=%.4f Brier=" % (r.ece, r.mce, r.nll))
    # an empty block: nan everywhere, never an exception
    e = Reliability.zeros(bins)
    assert all(math.isnan(v) for v in (e.ece, e.mce, e.nll, e.brier, e.accuracy, e.mean_conf))


def test_temper_host_properties():
    rng = np.random.Generator(np.random.PCG64(3))
    for K in (1, 2, 9, 17, 64):
        z = 2.0 * rng.standard_normal((200, K))
        p = np.exp(z - z.max(axis=1, keepdims=True))
        p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
        prev = None
        for T in (1 / 16, 0.5, 1.0, 2.03, 16.0):
            q, lab, conf, ent = temper_host(p, T)
            assert q.dtype == np.float32 and np.abs(q.astype(np.float64).sum(axis=1) - 1).max() <= K * 2.0 ** -23
            assert np.array_equal(lab, p.argmax(axis=1))                                    # the label is unchanged
            assert np.array_equal(conf, q.max(axis=1))
            p64 = p.astype(np.float64) ** (1.0 / T)
            np.testing.assert_allclose(q, p64 / p64.sum(axis=1, keepdims=True), rtol=2e-4, atol=1e-30)
            if prev is not None and K > 1:
                assert (ent >= prev - 1e-5).all() and ent.mean() > prev.mean()               # entropy rises with T
            prev = ent
        if K > 1:
            np.testing.assert_allclose(temper_host(p, 1.0)[0], p, rtol=1e-5, atol=1e-9)
    # rows that are no probability vectors: NaN everywhere; zeros stay exact zeros; ties keep the first maximum
    p = np.array([[0.5, 0.5, 0.0], [NAN, 0.5, 0.5], [0.0, 0.0, 0.0], [0.5, -0.1, 0.6], [0.25, 0.0, 0.75]], np.float32)
    q, lab, conf, ent = temper_host(p, 2.0)
    assert lab.tolist() == [0, 0, 0, 2, 2]
    assert q[0].tolist() == [0.5, 0.5, 0.0] and q[4, 1] == 0.0 and np.isnan(q[1:4]).all() and np.isnan(conf[1:4]).all()
    assert np.isnan(ent[1:4]).all() and ent[0] == pytest.approx(math.log(2), rel=1e-6)
    with pytest.raises(ValueError):
        temper_host(p, 0.0)


def test_nll_temps_host_against_float64():
    rng = np.random.Generator(np.random.PCG64(5))
    z = rng.standard_normal((300, 9))
    p = np.exp(2 * z - (2 * z).max(axis=1, keepdims=True))
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    truth = rng.integers(-1, 10, 300).astype(np.int64)
    p[7, :] = 0.0; p[8, truth[8] % 9] = 0.0; p[9, 0] = NAN
    truth[7:10] = np.clip(truth[7:10], 0, 8)
    betas = cal.coarse_betas()[::7]
    got = cal.nll_temps_host(p, truth, None, betas)
    known = (truth >= 0) & (truth < 9)
    assert got.shape == (2, len(betas)) and (got[1] == 3).all()
    ok = known.copy(); ok[7:10] = False
    l = np.log(p[ok].astype(np.float64))
    for s, b in enumerate(betas.astype(np.float64)):
        nll = np.log(np.exp(b * l).sum(axis=1)) - b * l[np.arange(ok.sum()), truth[ok]]
        assert abs(got[0, s] / FIX20 - nll.sum()) <= 1e-5 * nll.sum() + ok.sum() / FIX20
    rows = np.arange(299, -1, -1)
    assert np.array_equal(cal.nll_temps_host(p, truth[::-1].copy(), rows, betas), got)
    with pytest.raises(ValueError):
        cal.nll_temps_host(p, truth, None, [0.01])
    with pytest.raises(ValueError):
        cal.nll_temps_host(p, truth, None, np.ones(65))


def test_fit_grid_brackets_the_first_minimum_everywhere():
    coarse = cal.coarse_betas()
    assert coarse.dtype == np.float32 and coarse.shape == (64,) and coarse[0] == 1 / 16 and coarse[-1] == 16
    assert (np.diff(coarse) > 0).all()
    np.testing.assert_allclose(coarse[1:] / coarse[:-1], 256 ** (1 / 63), rtol=1e-6)
    assert cal.R2 == pytest.approx(cal.R1 ** (2 / 63)) and abs(cal.R2 - 1.0028) < 1e-4
    for j in (0, 1, 31, 62, 63):
        fine = cal.fine_betas(coarse, j)
        assert fine.dtype == np.float32 and fine.shape == (64,) and (np.diff(fine) > 0).all()
        assert fine.min() >= np.float32(1 / 16) and fine.max() <= np.float32(16)
        assert fine[0] == coarse[max(j - 1, 0)] and fine[-1] == coarse[min(j + 1, 63)] and fine[0] <= coarse[j] <= fine[-1]
        np.testing.assert_allclose(fine[1:] / fine[:-1], cal.R2 if 0 < j < 63 else cal.R1 ** (1 / 63), rtol=1e-5)
    # the search itself, on a convex function of beta with its minimum inside, at an end, and with a flat tie
    for target in (1 / 16, 0.07, 0.4931, 1.0, 7.7, 16.0):
        calls = []

        def sums(betas, target=target):
            calls.append(np.array(betas))
            b = np.asarray(betas, np.float64)
            return np.stack([np.rint((np.log(b) - math.log(target)) ** 2 * 2 ** 30).astype(np.int64), np.zeros(len(b), np.int64)])
        beta, col, cands = cal.fit_on(sums)
        assert len(calls) == 2 and all(len(c) == 64 for c in calls) and cands.shape == (128,)
        assert (cands >= np.float32(1 / 16)).all() and (cands <= np.float32(16)).all()
        assert max(beta / target, target / beta) <= cal.R2 and col.shape == (2,)
    assert cal.first_min([5, 3, 3, 4]) == 1


def test_predict_py_refuses_what_the_flags_cannot_mean():
    import predict
    parser = predict.build_parser()
    ok = lambda *a: predict.check_args(parser.parse_args(["--ckpt", "x.pt", *a]))
    for bad, word in ((("--net", "both", "--reliability"), "ONE prediction"), (("--net", "ema_both", "--temperature", "2"), "ONE prediction"),
                      (("--rel_bins", "20"), "belong to --reliability"), (("--save_reliability", "r.npz"), "belong to --reliability"),
                      (("--reliability", "--rel_bins", "0"), "1 .. 1024"), (("--reliability", "--rel_bins", "1025"), "1 .. 1024"),
                      (("--temperature", "0"), "finite T > 0"), (("--temperature", "-1"), "finite T > 0"),
                      (("--temperature", "nan"), "finite T > 0"), (("--temperature", "hot"), "finite T > 0"),
                      (("--calib_frac", "0.3"), "belong to --temperature fit"), (("--temperature", "2", "--calib_seed", "3"), "belong to --temperature fit"),
                      (("--temperature", "fit", "--calib_frac", "1"), "0 < F < 1"), (("--temperature", "fit", "--calib_frac", "0"), "0 < F < 1"),
                      (("--temperature", "fit", "--calib_seed", "-2"), "N >= 0")):
        with pytest.raises(SystemExit, match=word):
            ok(*bad)
    ok()
    ok("--reliability", "--rel_bins", "1024", "--save_reliability", "r.npz", "--net", "ensemble")
    ok("--temperature", "fit", "--calib_frac", "0.25", "--calib_seed", "7", "--smooth", "2", "--tta", "3")
    ok("--temperature", "2.03", "--net", "ema0")
    args = parser.parse_args(["--ckpt", "x.pt"])
    assert (args.reliability, args.rel_bins, args.save_reliability, args.temperature, args.calib_frac, args.calib_seed) == \
        (False, None, None, None, None, None)


def test_train_py_refuses_reliability_without_a_block_to_score():
    import train
    parser = train.build_parser()
    check = lambda *a: (lambda args: train.check_reliability_args(args, train.smooth_of(args)))(parser.parse_args(list(a)))
    with pytest.raises(SystemExit, match="--ensemble, --tta or --smooth"):
        check("--reliability")
    with pytest.raises(SystemExit, match="--no_eval"):
        check("--reliability", "--ensemble", "--no_eval")
    check("--reliability", "--ensemble"); check("--reliability", "--tta"); check("--reliability", "--smooth", "2"); check()
    args = parser.parse_args([])
    assert args.reliability is False and "reliability" not in train.saved_args(args)
    assert train.saved_args(parser.parse_args(["--reliability", "--ensemble"]))["reliability"] is True


def test_calibration_split_is_the_seeded_permutation():
    import train
    fit, held = train.calibration_split(11, 0.5, 1088)
    perm = np.random.default_rng(1088).permutation(11)
    assert len(fit) == round(0.5 * 11) and np.array_equal(fit, perm[:len(fit)]) and np.array_equal(held, perm[len(fit):])
    assert sorted(np.concatenate([fit, held]).tolist()) == list(range(11))
    assert np.array_equal(train.calibration_split(11, 0.5, 1088)[0], fit)
    assert not np.array_equal(train.calibration_split(11, 0.5, 1089)[0], fit)
