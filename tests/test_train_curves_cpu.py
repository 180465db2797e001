"""CPU: train.py's validation-curve record (``train.EvalCurve``) and the order of a checkpoint's ``extra``.

Every expected name, dtype, shape and value below is written out, not computed by the record: the three curves
(suffix '' -- the two networks --, '_ema' -- their teachers --, '_ens' -- the pair together, one row) are what the
checkpoints and the --save_eval files have always held, key for key and in that order (``checkpoint.save`` of a
permuted ``extra`` is another file)."""
import os

import numpy as np
import pytest
import torch

import train
from cmlpl_amd import checkpoint
from tests.test_checkpoint_cpu import HashEngine

K = 5
PAIR_ROWS = [[(0.5, 0.25, 0.125), (0.75, 0.5, 0.375)], [(0.625, 0.5, 0.25), (0.6875, 0.4375, 0.3125)]]   # [evaluation][net][OA, AA, Kappa]
ONE_ROWS = [(0.5, 0.25, 0.125), (0.625, 0.5, 0.25)]                                                        # [evaluation][OA, AA, Kappa]
EPOCHS = [1, 3]
CURVES = [("", 2), ("_ema", 2), ("_ens", None)]


def _cms(nets, evaluation):
    per = (K, K) if nets is None else (nets, K, K)
    return (np.arange(int(np.prod(per)), dtype=np.int64) + 1000 * evaluation).reshape(per)


def _filled(suffix, nets):
    curve = train.EvalCurve(suffix, nets)
    for i, epoch in enumerate(EPOCHS):
        curve.add(epoch, (ONE_ROWS if nets is None else PAIR_ROWS)[i], _cms(nets, i))
    return curve


@pytest.mark.parametrize("suffix,nets", CURVES)
def test_checkpoint_entries_of_an_empty_curve(suffix, nets):
    entries = train.EvalCurve(suffix, nets).checkpoint_entries(K)
    assert list(entries) == ["eval_epochs" + suffix, "eval_curve" + suffix, "eval_cms" + suffix]
    epochs, curve, cms = entries.values()
    assert epochs == [] and isinstance(epochs, list)
    assert curve.dtype == torch.float64 and tuple(curve.shape) == ((0, 3) if nets is None else (0, 2, 3))
    assert cms.dtype == torch.int64 and tuple(cms.shape) == ((0, K, K) if nets is None else (0, 2, K, K))


@pytest.mark.parametrize("suffix,nets", CURVES)
def test_checkpoint_entries_of_two_evaluations(suffix, nets):
    entries = _filled(suffix, nets).checkpoint_entries(K)
    assert list(entries) == ["eval_epochs" + suffix, "eval_curve" + suffix, "eval_cms" + suffix]
    epochs, curve, cms = entries.values()
    assert epochs == [1, 3] and all(type(e) is int for e in epochs)
    assert curve.dtype == torch.float64 and tuple(curve.shape) == ((2, 3) if nets is None else (2, 2, 3))
    assert cms.dtype == torch.int64 and tuple(cms.shape) == ((2, K, K) if nets is None else (2, 2, K, K))
    if nets is None:
        assert curve.tolist() == [[0.5, 0.25, 0.125], [0.625, 0.5, 0.25]]
        assert cms[1, 0].tolist() == [1000, 1001, 1002, 1003, 1004] and cms[0, 4, 4].item() == 24
    else:
        assert curve.tolist() == [[[0.5, 0.25, 0.125], [0.75, 0.5, 0.375]], [[0.625, 0.5, 0.25], [0.6875, 0.4375, 0.3125]]]
        assert cms[1, 0, 0].tolist() == [1000, 1001, 1002, 1003, 1004] and cms[0, 1, 4, 4].item() == 49


@pytest.mark.parametrize("suffix,nets,names", [("", 2, ["curve", "epochs", "cm"]),
                                               ("_ema", 2, ["curve_ema", "cm_ema", "epochs_ema"]),
                                               ("_ens", None, ["curve_ens", "cm_ens", "epochs_ens"])])
def test_npz_entries_keep_their_names_and_their_order(suffix, nets, names, tmp_path):
    entries = _filled(suffix, nets).npz_entries()
    assert list(entries) == names
    curve, cm, epochs = (entries[n + suffix] for n in ("curve", "cm", "epochs"))
    assert curve.dtype == np.float64 and curve.shape == ((2, 3) if nets is None else (2, 2, 3))
    assert cm.dtype == np.int64 and cm.shape == ((2, K, K) if nets is None else (2, 2, K, K))
    assert epochs.dtype == np.int64 and epochs.tolist() == [1, 3]
    np.savez(tmp_path / "e.npz", **entries)
    assert np.load(tmp_path / "e.npz").files == names              # the member order of the written file


@pytest.mark.parametrize("suffix,nets", CURVES)
def test_restore_gives_back_what_the_entries_hold(suffix, nets, tmp_path):
    extra = dict(epoch=3, **_filled(suffix, nets).checkpoint_entries(K))
    torch.save(extra, tmp_path / "x.pt")                           # through a file, as a checkpoint's extra goes
    back = train.EvalCurve(suffix, nets)
    back.restore(torch.load(tmp_path / "x.pt", weights_only=True))
    assert back.epochs == [1, 3] and all(type(e) is int for e in back.epochs)
    assert np.array(back.rows).tobytes() == np.array(ONE_ROWS if nets is None else PAIR_ROWS).tobytes()
    assert len(back.cms) == 2 and all(np.array_equal(back.cms[i], _cms(nets, i)) and back.cms[i].dtype == np.int64 for i in range(2))
    again = back.checkpoint_entries(K)                             # and a second leg writes the same entries
    assert all(torch.equal(again[k], extra[k]) if isinstance(extra[k], torch.Tensor) else again[k] == extra[k] for k in again)
    other = train.EvalCurve("_ema" if suffix != "_ema" else "_ens", nets)
    other.restore(extra)                                           # a file without this curve: a gap, not an error
    assert other.epochs == [] and other.rows == [] and other.cms == []


def test_best_line_is_the_first_of_equal_bests_in_percent():
    pair = _filled("", 2)
    assert pair.best_line(0) == "best validation: epoch 3 OA = 62.50" and pair.best_line(1) == "best validation1: epoch 1 OA = 75.00"
    assert _filled("_ens", None).best_line() == "best validation_ens: epoch 3 OA = 62.50"
    pair.add(4, [(0.625, 0.0, 0.0), (0.75, 0.0, 0.0)], _cms(2, 2))
    assert pair.best_line(0) == "best validation: epoch 3 OA = 62.50" and pair.best_line(1) == "best validation1: epoch 1 OA = 75.00"


PARENT_EXTRA = ["epoch", "num_batches", "loss_hist", "eval_epochs", "eval_curve", "eval_cms", "gen_state", "args", "run", "world"]
EMA_EXTRA = ["eval_epochs_ema", "eval_curve_ema", "eval_cms_ema"]
ENS_EXTRA = ["eval_epochs_ens", "eval_curve_ens", "eval_cms_ens"]


@pytest.mark.parametrize("flags,keys", [((), PARENT_EXTRA), (("--ema",), PARENT_EXTRA + EMA_EXTRA),
                                        (("--ensemble",), PARENT_EXTRA + ENS_EXTRA),
                                        (("--ema", "--ensemble"), PARENT_EXTRA + EMA_EXTRA + ENS_EXTRA)],
                         ids=["none", "ema", "ensemble", "both"])
def test_order_of_extra(flags, keys, tmp_path):
    """the late triples are there with their flag, --eval_every or not, behind the ten keys every checkpoint has"""
    args = train.build_parser().parse_args([
        "--synthetic", "B2", "--num_unlabel", "16", "--labeled_batch_size", "8", "--unlabeled_batch_size", "8",
        "--num_epochs", "1", "--print_per_batches", "2", "--no_eval", "--save_ckpt", str(tmp_path / "ck.pt"), *flags])
    train.main(args, make_engine=lambda shape, bt, btu, hp, ppb: HashEngine(shape, bt, btu, hp, ppb), device=torch.device("cpu"))
    extra = checkpoint.load(str(tmp_path / "ck.pt"))["extra"]
    assert list(extra) == keys
    for suffix, nets in CURVES:
        if "eval_curve" + suffix in extra:
            assert extra["eval_epochs" + suffix] == []
            assert tuple(extra["eval_curve" + suffix].shape) == ((0, 3) if nets is None else (0, 2, 3))
            assert tuple(extra["eval_cms" + suffix].shape) == ((0, 9, 9) if nets is None else (0, 2, 9, 9))
    assert os.listdir(tmp_path) == ["ck.pt"]
