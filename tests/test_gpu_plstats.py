"""GPU: the pseudo-label monitor (cmlpl_pl_stats / cmlpl_pl_stats_hard, TrainEngine(pl_monitor=True), train.py --pl_stats).

Everything here is an EQUALITY of integers.  The counters are sums of decisions; a decision is a comparison of fp32 values
the host restatement (cmlpl_amd.plstats.pl_stats_host, held to a scalar restatement in exact arithmetic by
tests/test_plstats_host.py) forms with the same operations in the same order, so kernel and host agree on every word.  The
random fixtures nevertheless keep every decision away from its threshold by far more than the error of an fp32 chain
evaluated any other way (K 2^-24 ~ 4e-6 at K = 64), and leave no case out to do so: rows are drawn again until the
margins hold, and the margins are asserted."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cmlpl_amd.plstats import PL_HEAD, PLCounts, graph_q, pl_size, pl_stats_hard_host, pl_stats_host
from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV
from tests.test_plstats_host import ADAP, NEG, POS, hand_block

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W8 = (40, 8, 8, 40, 5)
# no pairs; rows no multiple of 4, 64 or 256; K across 32; K filling the wave
SHAPES = ((1, 2), (5, 3), (64, 9), (65, 9), (128, 16), (130, 33), (257, 64))
GAP, MASK_MARGIN, Q_MARGIN = 1e-3, 1e-4, 1e-5


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _lib():
    from cmlpl_amd import _lib
    return _lib.load()


def _draw(rng, rows, K):
    z = 4.0 * rng.standard_normal((4, rows, K))
    e = np.exp(z - z.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


def _offending_rows(probs):
    """rows with a decision inside its margin, measured in fp64 on the float32 values the kernel reads"""
    p = probs.astype(np.float64)
    top = np.sort(p, axis=2)
    bad = np.zeros(p.shape[1], bool)
    if p.shape[2] > 1:
        bad |= ((top[:, :, -1] - top[:, :, -2]) < GAP).any(axis=0)
    bad |= (np.abs(top[:, :, -1] - ADAP) <= MASK_MARGIN).any(axis=0)
    q = p[1] @ p[0].T                                   # q[i][j] = p_s[i] . p_w[j]
    near = (np.abs(q - POS) <= Q_MARGIN) | (np.abs(q - NEG) <= Q_MARGIN)
    np.fill_diagonal(near, False)
    return bad | near.any(axis=1) | near.any(axis=0)


def make_case(btu, K, seed):
    """(probs float32 [4][btu][K], truth int64 [btu]) with every margin asserted; nothing is left out"""
    rng = np.random.Generator(np.random.PCG64(seed))
    probs = _draw(rng, btu, K)
    rounds = 0
    while True:
        bad = _offending_rows(probs)
        if not bad.any():
            break
        rounds += 1
        assert rounds <= 8, "the fixture does not converge"
        probs[:, bad] = _draw(rng, int(bad.sum()), K)
    assert not _offending_rows(probs).any()
    truth = probs[2].argmax(axis=1).astype(np.int64)
    wrong = rng.random(btu) < 0.25                      # a quarter of the rows: another class
    truth[wrong] = (truth[wrong] + rng.integers(1, K, int(wrong.sum()))) % K
    if btu >= 5:                                        # a few rows without a known truth, on both sides of the range
        out = rng.choice(btu, max(2, btu // 16), replace=False)
        truth[out[::2]], truth[out[1::2]] = -1, K
    return probs, truth, rounds


def _launch(probs, truth, idx, adap, pos, neg, counts=None):
    lib = _lib()
    _, btu, K = probs.shape
    dp = torch.from_numpy(np.ascontiguousarray(probs)).to(DEV)
    dt = torch.from_numpy(truth).to(DEV)
    di = None if idx is None else torch.from_numpy(idx).to(DEV)
    if counts is None:
        counts = torch.zeros(pl_size(K), dtype=torch.int64, device=DEV)
    rc = lib.cmlpl_pl_stats(dp.data_ptr(), btu, K, dt.data_ptr(), None if di is None else di.data_ptr(), adap, pos, neg,
                            counts.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return counts


def _differing(got: np.ndarray, want: np.ndarray):
    bad = np.nonzero(got != want)[0]
    return [(int(i), int(got[i]), int(want[i])) for i in bad[:12]]


# ------------------------------------------------------------------ a. the kernel against the definition
@pytest.mark.parametrize("btu,K", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_kernel_equals_the_definition_word_for_word(btu, K):
    probs, truth, rounds = make_case(btu, K, 1000 * btu + K)
    want = pl_stats_host(probs, truth, None, ADAP, POS, NEG)
    got = _launch(probs, truth, None, ADAP, POS, NEG).cpu().numpy()
    print("btu %d K %d: resampling rounds %d; sel %s of %s rows, pos %d neg %d of %d pairs" %
          (btu, K, rounds, want.sel.tolist(), want.rows.tolist(), want.pos, want.neg, want.pairs))
    assert got.shape == (PL_HEAD + 2 * K * K,)
    assert not _differing(got, want.counts), _differing(got, want.counts)
    assert want.sel.min() > 0 or btu == 1
    if btu >= 64:                                       # the fixture decides both ways
        assert want.pos > 0 and want.neg > 0 and want.sel.max() < want.rows.max() and want.hit.min() > 0
    # the same rows reached through an index vector
    rng = np.random.Generator(np.random.PCG64(btu))
    perm = rng.permutation(btu).astype(np.int64)
    spread = np.full(btu + 3, -1, np.int64)
    spread[perm] = truth                                # truth of row r lies at perm[r]
    got_idx = _launch(probs, spread, perm, ADAP, POS, NEG).cpu().numpy()
    assert not _differing(got_idx, want.counts), _differing(got_idx, want.counts)


def test_kernel_nan_rows_exact_ties_and_an_index_vector_with_repeats():
    probs, _ = hand_block()                             # a NaN row in p_w and one in p_w0, exact ties, max == adap_mask, q == pos_thr
    btu, K = probs.shape[1:]
    truth = np.array([2, 0, 1, -1, 3, 0, 1, 2, 0, 1, 5, -7], np.int64)
    idx = np.array([1, 1, 2, 3, 4, 0, 6, 0, 5], np.int64)                 # repeats; truths 0 0 1 -1 3 2 1 2 0: the hand block's
    want = pl_stats_host(probs, truth, idx, ADAP, POS, NEG)
    assert want.rows.tolist() == [7, 7] and want.nan_rows.tolist() == [2, 0] and want.nan_pairs == 6 and want.fixed[0] == 1
    got = _launch(probs, truth, idx, ADAP, POS, NEG).cpu().numpy()
    assert not _differing(got, want.counts), _differing(got, want.counts)
    # one ulp of threshold either way moves exactly the rows and pairs that sit on it
    for adap, pos in ((float(np.nextafter(np.float32(ADAP), np.float32(1))), POS), (ADAP, float(np.nextafter(np.float32(POS), np.float32(1))))):
        w = pl_stats_host(probs, truth, idx, adap, pos, NEG)
        assert w != want
        g = _launch(probs, truth, idx, adap, pos, NEG).cpu().numpy()
        assert not _differing(g, w.counts), _differing(g, w.counts)


def test_arguments_are_checked():
    lib = _lib()
    d = torch.zeros(64, dtype=torch.int64, device=DEV)
    f = torch.zeros(64, dtype=torch.float32, device=DEV)
    big = torch.zeros(pl_size(3), dtype=torch.int64, device=DEV)
    E_ARG = -1
    assert lib.cmlpl_pl_stats(f.data_ptr(), 0, 3, d.data_ptr(), None, 0.5, 0.8, 0.3, big.data_ptr(), _stream()) == E_ARG
    assert lib.cmlpl_pl_stats(f.data_ptr(), 2, 65, d.data_ptr(), None, 0.5, 0.8, 0.3, big.data_ptr(), _stream()) == E_ARG
    assert lib.cmlpl_pl_stats(f.data_ptr(), 2, 0, d.data_ptr(), None, 0.5, 0.8, 0.3, big.data_ptr(), _stream()) == E_ARG
    assert lib.cmlpl_pl_stats(None, 2, 3, d.data_ptr(), None, 0.5, 0.8, 0.3, big.data_ptr(), _stream()) == E_ARG
    assert lib.cmlpl_pl_stats(f.data_ptr(), 2, 3, None, None, 0.5, 0.8, 0.3, big.data_ptr(), _stream()) == E_ARG
    assert lib.cmlpl_pl_stats(f.data_ptr(), 2, 3, d.data_ptr(), None, 0.5, 0.8, 0.3, None, _stream()) == E_ARG
    assert lib.cmlpl_pl_stats(f.data_ptr(), 2, 3, d.data_ptr(), None, 0.5, 0.8, 0.3, big.data_ptr() + 4, _stream()) == E_ARG
    assert lib.cmlpl_pl_stats_hard(d.data_ptr(), 0, 3, d.data_ptr(), None, big.data_ptr(), _stream()) == E_ARG
    assert lib.cmlpl_pl_stats_hard(d.data_ptr(), 2, 65, d.data_ptr(), None, big.data_ptr(), _stream()) == E_ARG
    assert lib.cmlpl_pl_stats_hard(None, 2, 3, d.data_ptr(), None, big.data_ptr(), _stream()) == E_ARG
    torch.cuda.synchronize()
    assert not big.any()


# ------------------------------------------------------------------ b. accumulation
def test_launches_add_into_one_block():
    (pa, ta, _), (pb, tb, _) = make_case(65, 9, 7), make_case(130, 9, 8)
    counts = _launch(pa, ta, None, ADAP, POS, NEG)
    counts = _launch(pb, tb, None, 0.5, 0.7, 0.2, counts=counts)
    want = pl_stats_host(pa, ta, None, ADAP, POS, NEG) + pl_stats_host(pb, tb, None, 0.5, 0.7, 0.2)
    got = counts.cpu().numpy()
    assert want.launches == 2 and not _differing(got, want.counts), _differing(got, want.counts)
    assert PLCounts(got).launches == 2 and PLCounts(got) == want


# ------------------------------------------------------------------ c. hard labels
@pytest.mark.parametrize("btu,K", [(1, 2), (5, 3), (130, 9), (257, 64), (1000, 16)])
def test_hard_kernel_equals_the_definition(btu, K):
    lib = _lib()
    rng = np.random.Generator(np.random.PCG64(btu * 100 + K))
    truth = rng.integers(-1, K + 1, 2 * btu).astype(np.int64)              # unknown truths on both sides
    idx = rng.integers(0, 2 * btu, btu).astype(np.int64)
    pseudo = rng.integers(0, K, (2, btu)).astype(np.int64)
    agree = rng.random((2, btu)) < 0.5
    pseudo = np.where(agree, np.clip(truth[idx], 0, K - 1)[None], pseudo)
    pseudo[0, rng.integers(0, btu)] = K                                     # labels outside [0, K)
    pseudo[1, rng.integers(0, btu)] = -1
    pseudo[1, rng.integers(0, btu)] = 2 ** 40
    for use_idx in (idx, None):
        want = pl_stats_hard_host(pseudo, truth, use_idx, K)
        counts = torch.zeros(pl_size(K), dtype=torch.int64, device=DEV)
        dps, dt = torch.from_numpy(pseudo).to(DEV), torch.from_numpy(truth).to(DEV)
        di = None if use_idx is None else torch.from_numpy(use_idx).to(DEV)
        for _ in range(2):
            assert lib.cmlpl_pl_stats_hard(dps.data_ptr(), btu, K, dt.data_ptr(), None if di is None else di.data_ptr(),
                                           counts.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        got = counts.cpu().numpy()
        assert not _differing(got, (want + want).counts), _differing(got, (want + want).counts)
        assert want.rows[0] > 0 or btu < 5


# ------------------------------------------------------------------ d / e / f. the engine
BT = 8
SHARP = 24.0        # the classifier weights of the fixture are scaled up: an untrained network's softmax is flat, and a flat
#                     softmax passes no mask and joins no pair -- with peaky ones the mask and the graph decide both ways


def _hp(**kw):
    from cmlpl_amd import HyperParams
    return HyperParams(thr=0.6, num_epochs=2, **kw)      # adap_mask 0.6 in epoch 0, 0.6 exp(-1/8) in epoch 1


def _engine(method="cmlpl", **kw):
    from cmlpl_amd import NetShape, TrainEngine
    eng = TrainEngine(NetShape(*W8), BT, BT, _hp(), device=DEV, seed=11, hist_rows=16, method=method, **kw)
    s = O.NetShape(*W8)
    for net in range(2):
        sd = O.closed_form_params(s, 1 + net)
        sd["classifier.weight"] = sd["classifier.weight"] * SHARP
        eng.load_state_dict(net, sd)
    return eng


def _splits(rows, seed=900):
    s = O.NetShape(*W8)
    b = O.synthetic_batch(s, rows, rows, seed, with_noise=False, separable=1.0)
    d = lambda k: b[k].to(DEV).contiguous()
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    truth = torch.from_numpy(rng.integers(0, W8[4], rows).astype(np.int64)).to(DEV)
    return d("XPl"), d("Xl"), d("Y"), d("XPu"), d("Xu"), truth


def _adap(hp, epoch):
    return C.c_float(float(hp.thr * hp.adap_thr(epoch))).value


SCHED = [(0, 16), (0, 17), (0, 18), (0, 19)]            # the smoothing gate opens at batch_index 18 (> queue_batch = 17)


def test_engine_counts_what_the_step_left_and_leaves_the_step_alone():
    K, steps = W8[4], len(SCHED)
    XPl, Xl, Y, XPu, Xu, truth = _splits(steps * BT)
    idx = torch.arange(steps * BT, dtype=torch.int64, device=DEV)
    ridx = torch.flip(idx, [0]).contiguous()              # the unlabelled rows in another order than the labelled ones
    A, M = _engine(), _engine(pl_monitor=True)
    assert A.pl_block is None and M.pl_block.shape == (PL_HEAD + 2 * K * K,) and M.pl_block.dtype == torch.int64
    with pytest.raises(RuntimeError, match="pl_monitor"):
        A.pl_counts()
    with pytest.raises(RuntimeError, match="pl_monitor"):
        A.pl_reset()
    with pytest.raises(ValueError, match="unl_truth"):
        M.step(XPl, Xl, Y, XPu, Xu, 0, 16, lab_idx=idx[:BT], unl_idx=ridx[:BT])
    with pytest.raises(ValueError, match="unl_truth"):
        M.step(XPl, Xl, Y, XPu, Xu, 0, 16, lab_idx=idx[:BT], unl_idx=ridx[:BT], unl_truth=truth[:BT])     # the split's, not the batch's
    assert M.step_count == 0
    total = PLCounts.zeros(K)
    for k, (epoch, bi) in enumerate(SCHED):
        sl = slice(k * BT, (k + 1) * BT)
        A.step(XPl, Xl, Y, XPu, Xu, epoch, bi, lab_idx=idx[sl], unl_idx=ridx[sl])
        M.step(XPl, Xl, Y, XPu, Xu, epoch, bi, lab_idx=idx[sl], unl_idx=ridx[sl], unl_truth=truth)
        probs = M.debug_region("probs")[: 4 * BT * K].view(4, BT, K).cpu().numpy()
        want = pl_stats_host(probs, truth.cpu().numpy(), ridx[sl].cpu().numpy(), _adap(M.hp, epoch), M.hp.pos_thr, M.hp.neg_thr)
        got = M.pl_counts()
        sc = M.read_scalars()
        print("step %d: sel %s hit %s hit_raw %s pos %d neg %d | n_mask_w %g n_mask_s %g n_pos %g n_neg %g" %
              (k, want.sel.tolist(), want.hit.tolist(), want.hit_raw.tolist(), want.pos, want.neg, sc["n_mask_w"],
               sc["n_mask_s"], sc["n_pos"], sc["n_neg"]))
        assert got == total + want, _differing(got.counts, (total + want).counts)
        total = got
        # the step's own scalars: every truth is known and nothing is NaN
        assert want.rows.tolist() == [BT, BT] and want.nan_rows.tolist() == [0, 0] and want.nan_pairs == 0
        assert want.sel[0] == sc["n_mask_w"] and want.sel[1] == sc["n_mask_s"]
        assert want.pos + BT == sc["n_pos"] and want.neg == sc["n_neg"]
        smoothed = not np.array_equal(probs[0], probs[2])
        assert smoothed == M.hp.smooth_gate(epoch, bi)
        if not smoothed:
            assert want.fixed.tolist() == [0, 0] and want.broken.tolist() == [0, 0]
    assert total.launches == steps and 0 < total.sel.sum() < 2 * steps * BT and total.pos > 0 and total.neg > 0
    # the step is what it is without the monitor
    torch.cuda.synchronize()
    for name in ("params", "m", "v", "bank_feats", "bank_probs", "scalar_hist"):
        assert torch.equal(getattr(A, name), getattr(M, name)), name
    assert np.array_equal(A.loss_window(steps), M.loss_window(steps))
    # a batch given as its rows: the truth is the batch's
    sl = slice(0, BT)
    M.pl_reset()
    assert M.pl_counts() == PLCounts.zeros(K)
    M.step(XPl[sl], Xl[sl], Y[sl], XPu[sl], Xu[sl], 1, 0, unl_truth=truth[sl].contiguous())
    probs = M.debug_region("probs")[: 4 * BT * K].view(4, BT, K).cpu().numpy()
    assert M.pl_counts() == pl_stats_host(probs, truth[sl].cpu().numpy(), None, _adap(M.hp, 1), M.hp.pos_thr, M.hp.neg_thr)


def _epochs(eng, data, perms, replay):
    """two epochs of 20 rows in batches of 8, 8 and a short 4; ``replay``: the full batches behind the first step are
    graph replays.  Returns the counters read (and reset) behind each epoch."""
    XPl, Xl, Y, XPu, Xu, truth = data
    lab, unl = torch.zeros(20, dtype=torch.int64, device=DEV), torch.zeros(20, dtype=torch.int64, device=DEV)
    batches = [(0, 8), (8, 8), (16, 4)]
    graph, out = None, []
    for epoch in range(2):
        lab.copy_(perms[epoch][0]); unl.copy_(perms[epoch][1])
        if graph is not None:
            graph.program([(epoch, bi, off, off) for bi, (off, size) in enumerate(batches) if size == BT])
        for bi, (off, size) in enumerate(batches):
            if graph is not None and size == BT:
                graph.launch()
            else:
                eng.step(XPl, Xl, Y, XPu, Xu, epoch, bi, lab_idx=lab[off:off + size], unl_idx=unl[off:off + size], unl_truth=truth)
            if replay and graph is None:
                graph = eng.capture(XPl, Xl, Y, XPu, Xu, lab, unl, BT, BT, capacity=4, unl_truth=truth)
                graph.program([(epoch, b2, o2, o2) for b2, (o2, s2) in enumerate(batches) if b2 > bi and s2 == BT])
        out.append(eng.pl_counts())
        eng.pl_reset()
    if graph is not None:
        graph.close()
    return out


@pytest.mark.parametrize("method", ["cmlpl", "cps"])
def test_replayed_run_counts_what_the_eager_run_counts(method):
    data = _splits(20, seed=901)
    rng = np.random.Generator(np.random.PCG64(5))
    perms = [[torch.from_numpy(rng.permutation(20).astype(np.int64)).to(DEV) for _ in range(2)] for _ in range(2)]
    E, G = _engine(method, pl_monitor=True), _engine(method, pl_monitor=True)
    with pytest.raises(ValueError, match="unl_truth"):
        E.capture(*data[:5], perms[0][0], perms[0][1], BT, BT)
    eager, replayed = _epochs(E, data, perms, False), _epochs(G, data, perms, True)
    torch.cuda.synchronize()
    for name in ("params", "m", "v", "bank_feats", "bank_probs", "scalar_hist"):
        assert torch.equal(getattr(E, name), getattr(G, name)), name
    for epoch in range(2):
        a, b = eager[epoch], replayed[epoch]
        print(method, "epoch", epoch, a)
        assert a.launches == 3 and a.rows.tolist() == [20, 20]
        assert a == b, _differing(b.counts, a.counts)
    if method == "cmlpl":
        # the threshold of epoch 1 is another one, and the replays have read it from their programmed rows
        assert _adap(E.hp, 1) < _adap(E.hp, 0) and eager[0].pairs == 2 * 8 * 7 + 4 * 3
    else:
        assert eager[0].pairs == 0 and (eager[0].sel == eager[0].rows).all()


def test_cps_engine_counts_its_hard_labels():
    K = W8[4]
    XPl, Xl, Y, XPu, Xu, truth = _splits(2 * BT, seed=902)
    truth[3] = -1
    idx = torch.arange(2 * BT, dtype=torch.int64, device=DEV)
    eng = _engine("cps", pl_monitor=True)
    total = PLCounts.zeros(K)
    for k in range(2):
        sl = slice(k * BT, (k + 1) * BT)
        eng.step(XPl, Xl, Y, XPu, Xu, 0, k, lab_idx=idx[sl], unl_idx=idx[sl], unl_truth=truth)
        pseudo = eng.pseudo_labels().cpu().numpy()
        want = pl_stats_hard_host(pseudo, truth.cpu().numpy(), idx[sl].cpu().numpy(), K)
        total = total + want
        assert eng.pl_counts() == total, _differing(eng.pl_counts().counts, total.counts)
    assert total.rows.tolist() == [2 * BT - 1] * 2 and (total.sel == total.rows).all() and total.launches == 2


# ------------------------------------------------------------------ g. the command line
BASE = ["--synthetic", "W8", "--synthetic_scene", "--windows", "cube", "--num_unlabel", "72", "--labeled_batch_size", "16",
        "--unlabeled_batch_size", "16", "--print_per_batches", "2", "--num_epochs", "2", "--no_eval", "--thr", "0.3"]


def _train(d, tag, *extra):
    hist, ck = os.path.join(d, f"hist_{tag}.npy"), os.path.join(d, tag + "_{epoch}.pt")
    r = subprocess.run([sys.executable, "train.py", *BASE, "--save_loss_hist", hist, "--ckpt_every", "1", "--save_ckpt", ck, *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if " steps in " not in ln]       # (wall times)
    return lines, np.load(hist)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pl"))
    out, hist = _train(d, "S", "--pl_stats", "--save_pl", os.path.join(d, "S.npy"))
    return dict(dir=d, out=out, hist=hist, S=np.load(os.path.join(d, "S.npy")))


def test_train_py_prints_a_line_per_epoch_and_writes_the_blocks(runs):
    S, K = runs["S"], W8[4]
    assert S.shape == (2, PL_HEAD + 2 * K * K) and S.dtype == np.int64
    lines = [ln for ln in runs["out"] if "pl_stats" in ln]
    print("\n".join(lines))
    assert len(lines) == 2
    for e, ln in enumerate(lines):
        c = PLCounts(S[e])
        assert c.launches == 5 and c.rows.tolist() == [72, 72] and c.nan_rows.tolist() == [0, 0]
        assert c.pairs == 4 * 16 * 15 + 8 * 7
        assert ln.startswith("Epoch %d/2: pl_stats sel = %d/72 acc_sel = " % (e + 1, c.sel[0]))
        assert " sel1 = %d/72 " % c.sel[1] in ln and " pos = %d pos_precision = " % c.pos in ln and " neg = %d neg_precision = " % c.neg in ln
        assert " acc = %.2f acc_raw = %.2f " % (c.acc[0] * 100, c.acc_raw[0] * 100) in ln
    # epoch 1 runs without smoothing (5 batches, the gate is at 17), epoch 2 with it
    first, second = PLCounts(S[0]), PLCounts(S[1])
    assert first.fixed.tolist() == [0, 0] and first.broken.tolist() == [0, 0] and (first.hit == first.hit_raw).all()
    assert np.isfinite(runs["hist"]).all() and runs["hist"].shape == (10, 5)
    assert second.counts[:PL_HEAD].sum() > 0


def test_train_py_graph_run_writes_the_same_blocks(runs):
    d = runs["dir"]
    out, hist = _train(d, "G", "--pl_stats", "--save_pl", os.path.join(d, "G.npy"), "--graph")
    assert hist.tobytes() == runs["hist"].tobytes()
    assert np.array_equal(np.load(os.path.join(d, "G.npy")), runs["S"])
    assert [ln for ln in out if "pl_stats" in ln] == [ln for ln in runs["out"] if "pl_stats" in ln]


def test_train_py_resumed_run_writes_the_same_blocks(runs):
    from cmlpl_amd import checkpoint
    d = runs["dir"]
    out, hist = _train(d, "R", "--pl_stats", "--save_pl", os.path.join(d, "R.npy"), "--resume", os.path.join(d, "S_1.pt"))
    assert hist.tobytes() == runs["hist"].tobytes()
    assert np.array_equal(np.load(os.path.join(d, "R.npy")), runs["S"])
    a, b = checkpoint.load(os.path.join(d, "S_2.pt")), checkpoint.load(os.path.join(d, "R_2.pt"))
    assert torch.equal(a["extra"]["pl_curve"], b["extra"]["pl_curve"]) and torch.equal(a["extra"]["pl_curve"], torch.from_numpy(runs["S"]))
    assert torch.equal(checkpoint.load(os.path.join(d, "S_1.pt"))["extra"]["pl_curve"], torch.from_numpy(runs["S"][:1]))
    assert [ln for ln in out if "pl_stats" in ln] == [ln for ln in runs["out"] if "pl_stats" in ln][1:]


def test_train_py_without_the_flag_is_the_parents_run(runs):
    from cmlpl_amd import checkpoint
    from tests.test_gpu_ema import PARENT_ARGS, PARENT_EXTRA, PARENT_IDENTITY, PARENT_KEYS, PARENT_RUN
    d = runs["dir"]
    out, hist = _train(d, "P")
    assert hist.tobytes() == runs["hist"].tobytes()                  # the monitor has not moved the run beside it
    assert out == [ln for ln in runs["out"] if "pl_stats" not in ln]
    ck, with_pl = checkpoint.load(os.path.join(d, "P_2.pt")), checkpoint.load(os.path.join(d, "S_2.pt"))
    assert set(ck) == PARENT_KEYS and set(ck["extra"]) == PARENT_EXTRA and set(ck["extra"]["args"]) == PARENT_ARGS
    assert set(ck["extra"]["run"]) == PARENT_RUN and set(ck["identity"]) == PARENT_IDENTITY
    assert set(with_pl) == PARENT_KEYS and set(with_pl["extra"]) == PARENT_EXTRA | {"pl_curve"}
    assert set(with_pl["extra"]["args"]) == PARENT_ARGS | {"pl_stats", "save_pl"} and with_pl["identity"] == ck["identity"]
    for k in checkpoint.STATE_TENSORS:
        assert torch.equal(ck[k], with_pl[k]), k
