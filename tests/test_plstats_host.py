"""CPU: the pseudo-label monitor's host side -- ``pl_stats_host`` (the definition of include/cmlpl.h restated in numpy, what
tests/test_gpu_plstats.py holds the kernel to) against a hand-built block and an independent scalar restatement,
``PLCounts``, the ``pl_curve`` a checkpoint carries under ``--pl_stats`` (and its absence without), and the refusals on
several GPUs."""
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

from cmlpl_amd import checkpoint
from cmlpl_amd.plstats import PL_HEAD, PLCounts, graph_q, pl_size, pl_stats_hard_host, pl_stats_host
from tests.test_checkpoint_cpu import HashEngine

F = np.float32
NAN = np.nan
ADAP, POS, NEG = 0.6, 0.8, 0.3
BELOW = float(np.nextafter(F(0.6), F(0)))          # the float32 just under the threshold
# rows r: p_w (block 0), p_s (block 1), p_w0 (block 2), p_s0 (block 3), truth -- K = 3
HAND = [
    # r0: an exact tie in p_w (first maximum: class 0) and in p_w0 (class 1): smoothing FIXED the label; below the mask
    ([0.5, 0.5, 0.0], [0.9, 0.05, 0.05], [0.2, 0.4, 0.4], [0.9, 0.05, 0.05], 0),
    # r1: max == adap_mask exactly: selected.  Base1's target went from right (p_s0) to wrong (p_s): BROKEN
    ([0.6, 0.3, 0.1], [0.1, 0.8, 0.1], [0.6, 0.3, 0.1], [0.7, 0.2, 0.1], 0),
    # r2: one ulp under the mask: not selected
    ([BELOW, 0.3, 0.1], [0.05, 0.9, 0.05], [BELOW, 0.3, 0.1], [0.05, 0.9, 0.05], 1),
    # r3, r4: truth -1 and K: nothing anywhere, however confident the row
    ([0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], -1),
    ([1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], 3),
    # r5: a NaN in p_w0 only: a NaN row of direction 0, but its p_w is clean, so no pair is NaN
    ([0.1, 0.1, 0.8], [0.0, 0.1, 0.9], [NAN, 0.1, 0.8], [0.0, 0.1, 0.9], 2),
    # r6: a NaN in p_w: a NaN row of direction 0 AND q(i, 6) is NaN for every i
    ([NAN, 0.5, 0.5], [0.05, 0.9, 0.05], [0.3, 0.4, 0.3], [0.05, 0.9, 0.05], 1),
    # r7: confident and right in both directions; q(5, 7) = 0.86: a positive edge inside class 2
    ([0.0, 0.05, 0.95], [0.0, 0.05, 0.95], [0.0, 0.05, 0.95], [0.0, 0.05, 0.95], 2),
    # r8: confident and WRONG for Base (class 1, truth 0); q(1, 8) = 0.8f == pos_thr exactly
    ([0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], 0),
]


def hand_block():
    probs = np.array([[row[b] for row in HAND] for b in range(4)], dtype=F)
    return probs, np.array([row[4] for row in HAND], dtype=np.int64)


def _round32(x: Fraction) -> F:
    """the correct rounding of an exact rational to float32 (ties to even)"""
    f = F(float(x))
    cands = [np.nextafter(f, F(-np.inf)), f, np.nextafter(f, F(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(F(v).view(np.int32)) & 1))


def slow_counts(probs, truth, idx, adap, pos_thr, neg_thr):
    """the definition once more, one row and one pair at a time, with exact rational arithmetic under every fmaf"""
    _, btu, K = probs.shape
    adap, pos_thr, neg_thr = F(adap), F(pos_thr), F(neg_thr)
    t = [int(truth[r if idx is None else idx[r]]) for r in range(btu)]
    out = np.zeros(pl_size(K), np.int64)
    for d in range(2):
        for r in range(btu):
            if not 0 <= t[r] < K:
                continue
            p, p0 = probs[d, r], probs[2 + d, r]
            out[8 * d] += 1
            if np.isnan(p).any() or np.isnan(p0).any():
                out[8 * d + 1] += 1
                continue
            l = min(k for k in range(K) if p[k] == p.max())
            l0 = min(k for k in range(K) if p0[k] == p0.max())
            m = bool(p[l] >= adap)
            flags = (m, l0 == t[r], l == t[r], m and l == t[r], l0 != t[r] and l == t[r], l0 == t[r] and l != t[r])
            out[8 * d + 2: 8 * d + 8] += np.array(flags, dtype=np.int64)
            if m:
                out[PL_HEAD + (d * K + t[r]) * K + l] += 1
    for i in range(btu):
        for j in range(btu):
            if i == j or not 0 <= t[i] < K or not 0 <= t[j] < K:
                continue
            out[16] += 1
            ps, pw = probs[1, i], probs[0, j]
            if np.isnan(ps).any() or np.isnan(pw).any():
                out[17] += 1
                continue
            q = F(0)
            for k in range(K):
                q = _round32(Fraction(float(ps[k])) * Fraction(float(pw[k])) + Fraction(float(q)))
            if q >= pos_thr:
                out[18] += 1
                out[19] += t[i] == t[j]
            if q <= neg_thr:
                out[20] += 1
                out[21] += t[i] != t[j]
    out[22] = 1
    return out


def check_identities(c: PLCounts, known: int):
    """what holds for every block, whatever the inputs (section 1 of the definition)"""
    for d in range(2):
        assert c.rows[d] == known * c.launches
        assert c.hit[d] == c.hit_raw[d] + c.fixed[d] - c.broken[d]
        assert c.sel_hit[d] <= min(c.sel[d], c.hit[d]) and c.sel[d] + c.nan_rows[d] <= c.rows[d]
        assert c.cm[d].sum() == c.sel[d] and np.trace(c.cm[d]) == c.sel_hit[d]
    assert c.pairs == known * (known - 1) * c.launches
    assert c.pos_same <= c.pos and c.neg_diff <= c.neg and c.pos + c.neg + c.nan_pairs <= c.pairs
    assert c.counts[23:PL_HEAD].sum() == 0


def test_hand_built_block():
    probs, truth = hand_block()
    c = pl_stats_host(probs, truth, None, ADAP, POS, NEG)
    assert c.K == 3 and c.counts.shape == (PL_HEAD + 18,)
    # the row part, counted by hand (the comments of HAND)
    want = dict(rows=[7, 7], nan_rows=[2, 0], sel=[3, 7], hit_raw=[2, 7], hit=[3, 6], sel_hit=[2, 6], fixed=[1, 0], broken=[0, 1])
    for name, v in want.items():
        assert getattr(c, name).tolist() == v, name
    cm = np.zeros((2, 3, 3), np.int64)
    cm[0, 0, 0], cm[0, 2, 2], cm[0, 0, 1] = 1, 1, 1
    cm[1, 0, 0], cm[1, 0, 1], cm[1, 1, 1], cm[1, 2, 2] = 2, 1, 2, 2
    assert np.array_equal(c.cm, cm)
    assert c.gain.tolist() == [1, -1]
    # the pair part: 7 known rows; column 6 is NaN for the six other known rows
    q = graph_q(probs)
    assert q.dtype == F and q[1, 8] == F(0.8) and abs(float(q[5, 7]) - 0.86) < 1e-6 and np.isnan(q[:, 6]).all()
    assert c.pairs == 42 and c.nan_pairs == 6 and c.launches == 1
    assert c.pos > 0 and c.neg > 0 and 0 < c.pos_same < c.pos and c.neg_diff > 0
    check_identities(c, 7)
    # and every word against the scalar restatement
    assert np.array_equal(c.counts, slow_counts(probs, truth, None, ADAP, POS, NEG))
    # q(1, 8) == pos_thr counts as positive; one ulp more of threshold and it does not
    up = pl_stats_host(probs, truth, None, ADAP, float(np.nextafter(F(POS), F(1))), NEG)
    assert up.pos == c.pos - 1 and up.pos_same == c.pos_same - 1                    # (rows 1 and 8 are both class 0)
    # and the mask one ulp higher drops row 1 of direction 0
    hi = pl_stats_host(probs, truth, None, float(np.nextafter(F(ADAP), F(1))), POS, NEG)
    assert hi.sel.tolist() == [2, 7] and hi.cm[0, 0, 0] == 0


def test_index_vector_with_repeats_and_random_blocks():
    rng = np.random.Generator(np.random.PCG64(3))
    for btu, K in ((1, 2), (5, 3), (13, 9)):
        z = rng.standard_normal((4, btu, K)) * 3
        e = np.exp(z - z.max(axis=2, keepdims=True))
        probs = (e / e.sum(axis=2, keepdims=True)).astype(F)
        truth = rng.integers(-1, K + 1, 4 * btu).astype(np.int64)
        idx = rng.integers(0, 4 * btu, btu).astype(np.int64)
        idx[-1] = idx[0]                                                            # a repeat
        c = pl_stats_host(probs, truth, idx, 0.5, 0.6, 0.2)
        assert np.array_equal(c.counts, slow_counts(probs, truth, idx, 0.5, 0.6, 0.2)), (btu, K)
        t = truth[idx]
        check_identities(c, int(((t >= 0) & (t < K)).sum()))
    assert pl_stats_host(probs[:, :1], truth, None, 0.5, 0.6, 0.2).pairs == 0       # one row: no pairs


def test_hard_labels():
    truth = np.array([0, 1, 2, -1, 3, 1, 2], np.int64)
    pseudo = np.array([[0, 2, 2, 1, 1, 3, -1], [1, 1, 2, 0, 0, 1, 2]], np.int64)
    c = pl_stats_hard_host(pseudo, truth, None, 3)
    assert c.rows.tolist() == [5, 5] and c.nan_rows.tolist() == [2, 0] and c.sel.tolist() == [3, 5]
    assert c.hit.tolist() == [2, 4] and c.hit_raw.tolist() == [2, 4] and c.sel_hit.tolist() == [2, 4]
    assert c.fixed.tolist() == [0, 0] and c.broken.tolist() == [0, 0]
    assert c.pairs == c.pos == c.neg == 0 and c.launches == 1
    cm = np.zeros((2, 3, 3), np.int64)
    cm[0, 0, 0], cm[0, 1, 2], cm[0, 2, 2] = 1, 1, 1
    cm[1, 0, 1], cm[1, 1, 1], cm[1, 2, 2] = 1, 2, 2
    assert np.array_equal(c.cm, cm)
    idx = np.array([6, 6, 0], np.int64)
    d = pl_stats_hard_host(pseudo[:, :3], truth, idx, 3)                            # truths 2, 2, 0
    assert d.rows.tolist() == [3, 3] and d.hit.tolist() == [1, 0] and d.cm[0, 2, 0] == 1 and d.cm[0, 2, 2] == 1


def test_rates_and_zero_denominators():
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                              # no divide warning either
        z = PLCounts.zeros(3)
        for name in ("sel_rate", "acc_raw", "acc", "acc_sel"):
            assert np.isnan(getattr(z, name)).all() and getattr(z, name).shape == (2,), name
        assert np.isnan(z.pos_precision) and np.isnan(z.neg_precision) and isinstance(z.pos_precision, float)
        assert np.isnan(z.class_precision).all() and z.class_precision.shape == (2, 3)
        assert z.gain.tolist() == [0, 0]
        probs, truth = hand_block()
        c = pl_stats_host(probs, truth, None, ADAP, POS, NEG)
        assert c.sel_rate.tolist() == [3 / 7, 1.0] and c.acc.tolist() == [3 / 7, 6 / 7] and c.acc_raw.tolist() == [2 / 7, 1.0]
        assert c.acc_sel.tolist() == [2 / 3, 6 / 7]
        assert c.pos_precision == c.pos_same / c.pos and c.neg_precision == c.neg_diff / c.neg
        cp = c.class_precision
        assert cp[0, 0] == 1.0 and cp[0, 1] == 0.0 and cp[0, 2] == 1.0 and cp[1, 1] == 2 / 3
        # selected nothing in direction 0: its rates are nan, the other direction's are not
        none = pl_stats_host(probs, truth, None, 2.0, POS, NEG)
        assert none.sel.tolist() == [0, 0] and np.isnan(none.acc_sel).all() and not np.isnan(none.acc).any()
    two = c + c
    assert two.launches == 2 and np.array_equal(two.counts, 2 * c.counts) and two == c + c and two != c
    check_identities(two, 7)
    assert (c + PLCounts.zeros(3)) == c
    with pytest.raises(ValueError):
        c + PLCounts.zeros(4)
    with pytest.raises(ValueError):
        PLCounts(np.zeros(PL_HEAD + 19, np.int64))
    with pytest.raises(ValueError):
        PLCounts(np.zeros(PL_HEAD + 18, np.int32))
    with pytest.raises(AttributeError):
        c.no_such_field


# ------------------------------------------------------------------ train.py's loop: the curve in the checkpoint
class MonitorEngine(HashEngine):
    """TEST-ONLY: HashEngine with the monitor's three calls; its "pseudo-labels" are a function of the truth and the step"""
    K = 9

    def __init__(self, *a):
        super().__init__(*a)
        self.block = PLCounts.zeros(self.K)

    def step(self, XPl, Xl, Y, XPu, Xu, epoch, batch_index, unl_truth=None):
        assert unl_truth is not None and unl_truth.shape[0] == Xu.shape[0]
        t = unl_truth.numpy()
        pseudo = np.stack([(t + (np.arange(len(t)) + self.step_count) % 3) % self.K, t])
        self.block = self.block + pl_stats_hard_host(pseudo, t, None, self.K)
        super().step(XPl, Xl, Y, XPu, Xu, epoch, batch_index)

    def pl_counts(self):
        return self.block

    def pl_reset(self):
        self.block = PLCounts.zeros(self.K)


def _run(tmp_path, *extra, monitor=True):
    import train
    args = train.build_parser().parse_args([
        "--synthetic", "B2", "--num_unlabel", "40", "--labeled_batch_size", "8", "--unlabeled_batch_size", "8",
        "--num_epochs", "4", "--print_per_batches", "2", "--no_eval", *extra])
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        return train.main(args, make_engine=lambda shape, bt, btu, hp, ppb: (MonitorEngine if monitor else HashEngine)(shape, bt, btu, hp, ppb),
                          device=torch.device("cpu"))
    finally:
        os.chdir(cwd)


def test_pl_curve_round_trip_and_absence(tmp_path, capsys):
    plain = _run(tmp_path, "--save_ckpt", "plain.pt", monitor=False)
    out_plain = capsys.readouterr().out
    assert "pl_stats" not in out_plain
    straight = _run(tmp_path, "--pl_stats", "--save_pl", "S.npy", "--ckpt_every", "2", "--save_ckpt", "ck{epoch}.pt")
    out = capsys.readouterr().out
    assert straight.tobytes() == plain.tobytes()
    lines = [ln for ln in out.splitlines() if "pl_stats" in ln]
    assert len(lines) == 4 and all(ln.startswith("Epoch %d/4: pl_stats sel = " % (e + 1)) for e, ln in enumerate(lines))
    timed = lambda text, skip=(): [ln for ln in text.splitlines() if " steps in " not in ln and not any(w in ln for w in skip)]
    assert timed(out, skip=("pl_stats",)) == timed(out_plain)                       # nothing else moved
    S = np.load(str(tmp_path / "S.npy"))
    assert S.shape == (4, PL_HEAD + 2 * 81) and S.dtype == np.int64 and (S[:, 22] == 5).all() and (S[:, 0] == 40).all()
    ck2, ck4 = checkpoint.load(str(tmp_path / "ck2.pt")), checkpoint.load(str(tmp_path / "ck4.pt"))
    assert torch.equal(ck2["extra"]["pl_curve"], torch.from_numpy(S[:2])) and torch.equal(ck4["extra"]["pl_curve"], torch.from_numpy(S))
    assert ck2["extra"]["args"]["pl_stats"] is True
    # the resumed run's curve is the straight run's
    _run(tmp_path, "--pl_stats", "--save_pl", "R.npy", "--resume", "ck2.pt", "--save_ckpt", "again{epoch}.pt")
    assert np.array_equal(np.load(str(tmp_path / "R.npy")), S)
    assert torch.equal(checkpoint.load(str(tmp_path / "again4.pt"))["extra"]["pl_curve"], ck4["extra"]["pl_curve"])
    # without the flag: no curve, no trace of the flags among the saved arguments
    ck = checkpoint.load(str(tmp_path / "plain.pt"))
    assert "pl_curve" not in ck["extra"] and "pl_stats" not in ck["extra"]["args"] and "save_pl" not in ck["extra"]["args"]
    assert set(ck4["extra"]) == set(ck["extra"]) | {"pl_curve"}
    assert ck4["extra"]["run"] == ck["extra"]["run"]                                # the monitor is no part of the run's record
    with pytest.raises(SystemExit) as e:
        _run(tmp_path, "--save_pl", "x.npy", monitor=False)
    assert "--save_pl belongs to --pl_stats" in str(e.value)


# ------------------------------------------------------------------ several GPUs
def test_sharded_engine_and_launcher_run_refuse(monkeypatch):
    from cmlpl_amd import NetShape
    from cmlpl_amd.distributed import DistTrainEngine
    with pytest.raises(ValueError, match="pl_monitor"):
        DistTrainEngine(NetShape(), 16, 16, pl_monitor=True)
    import train
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("LOCAL_RANK", "1")

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch.cuda, "set_device", boom)
    args = train.build_parser().parse_args(["--pl_stats", "--synthetic", "B2", "--no_eval"])
    with pytest.raises(SystemExit) as e:
        train.main(args)
    assert "--pl_stats runs on one GPU" in str(e.value) and "\n" not in str(e.value)


def test_launcher_run_of_the_driver_ends_at_once():
    """as a real process with the rendezvous variables of a two-rank job set: out before any device or process group"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "train.py", "--synthetic", "B2", "--pl_stats", "--no_eval"], cwd=root, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--pl_stats runs on one GPU" in r.stderr
    import train
    help_text = " ".join(train.build_parser().format_help().split())
    assert "--pl_stats" in help_text and "it needs --synthetic_scene" in help_text
