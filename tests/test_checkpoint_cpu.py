"""CPU: the checkpoint file (cmlpl_amd/checkpoint.py) and train.py's --save_ckpt / --ckpt_every / --resume.

The file: a round trip keeps every tensor bit for bit (NaN payloads and flag words included) and reads back with
``weights_only=True``; a write that dies midway leaves the previous file and no temporary file; an unknown format
version and every differing identity field are refused by name.  The loop: ``train.main`` around a small deterministic
stand-in engine whose "loss" is a hash of the rows it was handed and of its own counters -- a wrong permutation, a
wrong step number or a lost piece of state after a resume shows in ``loss_hist``."""
import os
import warnings

import numpy as np
import pytest
import torch

from cmlpl_amd import HyperParams, NetShape, checkpoint


def _state(seed=0):
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (2, 40), generator=g, dtype=torch.int64).to(torch.int32)
    ident = checkpoint.make_identity(NetShape(103, 11, 11, 103, 9), HyperParams(), 128, 128, 1280, "0123456789abcdef", 6)
    return dict(params=bits.view(torch.float32).clone(),                  # every bit pattern: NaNs, denormals, -0
                m=torch.randn(2, 40, generator=g), v=torch.rand(2, 40, generator=g),
                bank_feats=torch.randn(2, 6, 8, generator=g), bank_probs=torch.rand(2, 6, 9, generator=g),
                range_flags=torch.tensor([[1] + [0] * 15, [0] * 16], dtype=torch.int32),
                ptr=[256, 512], adam_t=77, step_count=78, seed=1088, identity=ident,
                Base={"conv0.weight": torch.randn(4, 3, 1, 1, generator=g)}, Base1={"conv0.weight": torch.randn(4, 3, 1, 1, generator=g)})


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.contiguous().view(torch.uint8).flatten().tolist() == \
        b.contiguous().view(torch.uint8).flatten().tolist()


def test_file_round_trip_is_bit_exact_and_weights_only(tmp_path):
    st = _state()
    gen = torch.Generator().manual_seed(5)
    torch.randperm(100, generator=gen)
    extra = dict(epoch=3, loss_hist=torch.from_numpy(np.random.default_rng(1).standard_normal((12, 5))),
                 gen_state=gen.get_state(), args=dict(lr=5e-4, graph=False, synthetic="B2", save_ckpt=None))
    path = tmp_path / "a.ckpt"
    checkpoint.save(str(path), st, extra)
    assert sorted(os.listdir(tmp_path)) == ["a.ckpt"]
    raw = torch.load(str(path), weights_only=True)                        # no pickled objects in the file
    assert raw["format_version"] == checkpoint.FORMAT_VERSION
    ck = checkpoint.load(str(path))
    for k in checkpoint.STATE_TENSORS:
        assert _same_bits(ck[k], st[k]), k
    for k in ("Base", "Base1"):
        assert list(ck[k]) == list(st[k]) and all(_same_bits(ck[k][n], st[k][n]) for n in st[k])
    assert ck["ptr"] == [256, 512] and (ck["adam_t"], ck["step_count"], ck["seed"]) == (77, 78, 1088)
    assert ck["identity"] == st["identity"] and isinstance(ck["identity"]["hp"], dict)
    assert ck["extra"]["epoch"] == 3 and ck["extra"]["args"] == extra["args"]
    assert _same_bits(ck["extra"]["loss_hist"], extra["loss_hist"])
    gen2 = torch.Generator()
    gen2.set_state(ck["extra"]["gen_state"])
    assert torch.equal(torch.randperm(50, generator=gen2), torch.randperm(50, generator=gen))


def test_a_write_that_fails_midway_keeps_the_previous_file(tmp_path, monkeypatch):
    path = tmp_path / "a.ckpt"
    checkpoint.save(str(path), _state(1), dict(epoch=1))
    before = path.read_bytes()

    def dies(obj, f, *a, **k):
        f.write(b"half a file")
        f.flush()
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", dies)
    with pytest.raises(OSError, match="disk full"):
        checkpoint.save(str(path), _state(2), dict(epoch=2))
    monkeypatch.undo()
    assert sorted(os.listdir(tmp_path)) == ["a.ckpt"] and path.read_bytes() == before
    assert checkpoint.load(str(path))["extra"]["epoch"] == 1


def test_unknown_format_version_is_a_clear_error(tmp_path):
    path = str(tmp_path / "v.ckpt")
    torch.save({"format_version": checkpoint.FORMAT_VERSION + 1, "params": torch.zeros(2)}, path)
    with pytest.raises(checkpoint.CheckpointError, match=f"version {checkpoint.FORMAT_VERSION + 1}"):
        checkpoint.load(path)
    torch.save({"params": torch.zeros(2)}, path)
    with pytest.raises(checkpoint.CheckpointError, match="format_version"):
        checkpoint.load(path)


def _ident(**kw):
    shape = {k: kw.pop(k) for k in list(kw) if k in ("C", "H", "W", "bands", "K")}
    hp = {k: kw.pop(k) for k in list(kw) if k in HyperParams.__dataclass_fields__}
    base = dict(bt=128, btu=128, Q=1280, source_hash="0123456789abcdef", abi=6)
    base.update(kw)
    return checkpoint.make_identity(NetShape(**{**dict(C=103, H=11, W=11, bands=103, K=9), **shape}), HyperParams(**hp), **{
        "bt_global": base["bt"], "btu_global": base["btu"], "Q": base["Q"], "source_hash": base["source_hash"], "abi": base["abi"]})


MISMATCHES = [("shape." + k, {k: v}) for k, v in (("C", 60), ("H", 9), ("W", 9), ("bands", 200), ("K", 16))] + \
             [("hp." + k, {k: (v + 1 if isinstance(v, int) else v * 0.5 + 0.01)}) for k, v in
              ((f, getattr(HyperParams(), f)) for f in HyperParams.__dataclass_fields__)] + \
             [("bt", dict(bt=64)), ("btu", dict(btu=256)), ("Q", dict(Q=640)), ("abi", dict(abi=5))]


@pytest.mark.parametrize("name,change", MISMATCHES, ids=[n for n, _ in MISMATCHES])
def test_each_mismatching_identity_field_is_named(name, change):
    with pytest.raises(ValueError) as e:
        checkpoint.check_identity(_ident(**change), _ident())
    assert name + ":" in str(e.value)
    assert len(checkpoint.identity_differences(_ident(**change), _ident())) == 1


def test_every_differing_field_is_listed_and_the_source_hash_only_warns():
    with pytest.raises(ValueError) as e:
        checkpoint.check_identity(_ident(K=16, lr=1e-3, Q=640), _ident())
    assert all(n in str(e.value) for n in ("shape.K:", "hp.lr:", "Q:"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        checkpoint.check_identity(_ident(), _ident())
    with pytest.warns(UserWarning, match="source hash"):
        checkpoint.check_identity(_ident(source_hash="f" * 16), _ident())


# ------------------------------------------------------------------ train.py's loop around a stand-in engine
class HashEngine:
    """TEST-ONLY: the part of the engine interface train.py's loop uses, on CPU.  Its state is a small vector ``w`` and
    the step counter; a step folds a hash of the batch rows, the epoch / batch index and the counter into ``w``, and the
    logged row is made of all of them."""

    def __init__(self, shape, bt, btu, hp, hist_rows):
        self.shape, self.hp, self.bt, self.btu = shape, hp, bt, btu
        self.hist_rows, self.rows, self.step_count = hist_rows, [], 0
        self.w = torch.zeros(4, dtype=torch.float64)
        self.steps_here = 0

    def init_params_default(self, seed=1088):
        self.w = torch.arange(4, dtype=torch.float64) + seed

    def step(self, XPl, Xl, Y, XPu, Xu, epoch, batch_index):
        d = lambda t: float(t.double().sum())
        h = d(XPl) + 3.0 * d(Xl) + 7.0 * d(Y) + 11.0 * d(XPu) + 13.0 * d(Xu)
        self.w = 0.5 * self.w + torch.tensor([h, epoch, batch_index, self.step_count], dtype=torch.float64) * self.hp.lr * 1e3
        self.rows.append(torch.tensor([float(self.w.sum()), h, float(self.w[0]), float(self.w[3]), float(self.step_count)],
                                      dtype=torch.float64))
        self.step_count += 1
        self.steps_here += 1

    def loss_window(self, k):
        assert 1 <= k <= self.hist_rows and k <= len(self.rows)
        return torch.stack(self.rows[-k:]).numpy()

    def state_dict(self, net):
        return {"w": self.w.clone()}

    def checkpoint_state(self, on_device=False, into=None):
        return dict(w=self.w.clone(), step_count=self.step_count, identity=dict(lr=float(self.hp.lr)))

    def load_checkpoint_state(self, state):
        if state["identity"]["lr"] != float(self.hp.lr):
            raise ValueError("hp.lr differs")
        self.w, self.step_count = state["w"].clone(), int(state["step_count"])


def _run(tmp_path, *extra):
    import train
    engines = []

    def make(shape, bt, btu, hp, ppb):
        engines.append(HashEngine(shape, bt, btu, hp, ppb))
        return engines[-1]
    args = train.build_parser().parse_args([
        "--synthetic", "B2", "--num_unlabel", "40", "--labeled_batch_size", "8", "--unlabeled_batch_size", "8",
        "--num_epochs", "4", "--print_per_batches", "2", "--no_eval", *extra])
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        hist = train.main(args, make_engine=make, device=torch.device("cpu"))
    finally:
        os.chdir(cwd)
    return hist, engines[0]


def test_resume_continues_the_run_exactly(tmp_path):
    plain, _ = _run(tmp_path)
    assert plain.shape == (20, 5) and len({tuple(r) for r in plain}) == 20
    straight, eng = _run(tmp_path, "--ckpt_every", "2", "--save_ckpt", "ck{epoch}.pt")
    assert np.array_equal(plain, straight)                                 # saving does not disturb the run
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("ck")) == ["ck2.pt", "ck4.pt"]
    ck = checkpoint.load(str(tmp_path / "ck2.pt"))
    assert ck["extra"]["epoch"] == 2 and ck["step_count"] == 10 and tuple(ck["extra"]["loss_hist"].shape) == (10, 5)
    resumed, eng2 = _run(tmp_path, "--resume", "ck2.pt", "--save_ckpt", "again{epoch}.pt")
    assert eng2.steps_here == 10 and eng2.step_count == 20
    assert resumed.tobytes() == straight.tobytes()
    # the file written at the end of the resumed leg is the file of the straight run
    a, b = checkpoint.load(str(tmp_path / "ck4.pt")), checkpoint.load(str(tmp_path / "again4.pt"))
    assert torch.equal(a["w"], b["w"]) and torch.equal(a["extra"]["loss_hist"], b["extra"]["loss_hist"])
    assert torch.equal(a["extra"]["gen_state"], b["extra"]["gen_state"])


def test_resuming_a_finished_run_takes_no_step(tmp_path):
    straight, _ = _run(tmp_path, "--save_ckpt", "ck{epoch}.pt")
    assert os.listdir(tmp_path) == ["ck4.pt"]
    hist, eng = _run(tmp_path, "--resume", "ck4.pt")
    assert eng.steps_here == 0 and eng.step_count == 20
    assert hist.tobytes() == straight.tobytes()


def test_a_differing_hyper_parameter_stops_the_resume_and_is_named(tmp_path):
    _run(tmp_path, "--ckpt_every", "2", "--save_ckpt", "ck{epoch}.pt")
    with pytest.raises(SystemExit) as e:
        _run(tmp_path, "--resume", "ck2.pt", "--lr", "0.001")
    assert e.value.code not in (0, None) and "lr:" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        _run(tmp_path, "--resume", "ck2.pt", "--num_epochs", "6", "--noise", "0.25")
    assert "num_epochs:" in str(e.value.code) and "noise:" in str(e.value.code) and "lr:" not in str(e.value.code)


def test_save_best_needs_eval_every_and_ckpt_every_needs_a_path(tmp_path):
    for flags in (("--save_best", "b.pt"), ("--ckpt_every", "2")):
        with pytest.raises(SystemExit) as e:
            _run(tmp_path, *flags)
        assert e.value.code not in (0, None)


def test_predict_shares_the_evaluation_of_train():
    import predict
    import train
    assert predict.evaluate_whole is train.evaluate_whole
    a = predict.build_parser().parse_args(["--ckpt", "x.pt", "--synthetic", "B2", "--net", "both"])
    assert (a.ckpt, a.synthetic, a.net, a.out) == ("x.pt", "B2", "both", None)
