"""GPU: the connected-region flags of the drivers (train.py / predict.py --sieve, --sp_connect) on the synthetic B2 scene, one
epoch, from a checkpoint made here.  What the drivers write is held to the definitions on the host
(cmlpl_amd.regions.sieve_host / connect_segments_host) exactly."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cmlpl_amd.regions import cc_label_host, connect_segments_host, sieve_host
from tests.test_gpu_superpixel_cli import COLS, ROWS, RUN, _oa_tags, _py, _timeless, scene  # noqa: F401  (scene: a fixture)

pytestmark = pytest.mark.gpu
LINE = re.compile(r"^sieve: components=(\d+) small=(\d+) relabelled=(\d+) passes_used=(\d+) components_after=(\d+)$")
CONNECT = re.compile(r"^superpixel connectivity: components_before=(\d+) fragments_merged=(\d+) segments=(\d+)$")
PREDICT = ["--synthetic", "B2", "--net", "ensemble"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sv"))
    f = lambda name: os.path.join(d, name)
    # (a checkpoint records the run's command line, paths included: both runs write the SAME paths, one after the other)
    files = ["--save_loss_hist", f("hist.npy"), "--save_ckpt", f("run.pt")]
    plain = _py("train.py", *RUN, *files)
    for name in ("hist.npy", "run.pt"):
        os.replace(f(name), f("plain_" + name))
    sieved = _py("train.py", *RUN, "--sieve", "4", *files)
    raw = _py("predict.py", "--ckpt", f("run.pt"), *PREDICT, "--out", f("lab0.npy"), "--proba", f("p.npy"), "--confidence", f("c0.npy"))
    return dict(sieved=sieved, plain=plain, raw=raw, f=f)


def _line(lines, labels, min_size, conn, passes):
    """the one ``sieve:`` line of ``lines`` against the definition on ``labels``; returns the definition's result"""
    got = [LINE.match(ln) for ln in lines if ln.startswith("sieve:")]
    assert len(got) == 1 and got[0] is not None, [ln for ln in lines if ln.startswith("sieve")]
    ref = sieve_host(labels, ROWS, COLS, min_size, conn, passes)
    s = ref["stats"].astype(np.int64)
    want = (s[0, 0], s[0, 1], s[:, 3].sum(), (s[:, 3] > 0).sum(), cc_label_host(ref["out"], ROWS, COLS, conn)["M"])
    assert tuple(int(v) for v in got[0].groups()) == tuple(int(v) for v in want)
    return ref


def test_train_adds_exactly_one_block_and_leaves_the_run_alone(runs):
    out, plain, f = runs["sieved"], runs["plain"], runs["f"]
    assert _oa_tags(out) == [" OA", " OA1", " OA_ens_sv"] and _oa_tags(plain) == [" OA", " OA1"]
    assert sum(ln.startswith("producerA_ens_sv:") for ln in out) == 1 and sum(ln.startswith("AA_ens_sv=") for ln in out) == 1
    assert sum("sieve time ==" in ln and "min_size 4" in ln for ln in out) == 1
    assert np.load(f("hist.npy")).tobytes() == np.load(f("plain_hist.npy")).tobytes()         # loss_hist bit-equal
    assert open(f("run.pt"), "rb").read() == open(f("plain_run.pt"), "rb").read()              # the checkpoint, every byte
    assert not any("sieve" in ln or "_sv" in ln or "connectivity" in ln for ln in plain)
    i = next(k for k, ln in enumerate(out) if ln.startswith("ensemble inference time"))
    assert _timeless(out[:i]) == _timeless(plain) and len(out) - i <= 12                       # every other line as it was
    ref = _line(out, np.load(f("lab0.npy")), 4, 4, 4)                                          # the same networks, the same map
    oa = 100 * (ref["out"] == np.asarray(scene_truth())).mean()
    assert [ln for ln in out if ln.startswith(" OA_ens_sv=")][0].startswith(" OA_ens_sv=%.2f," % oa)


def scene_truth():
    import train
    from hsi_loader import SyntheticScene
    return SyntheticScene(train.SYNTH["B2"], ROWS, COLS, seed=3).Y.numpy()


def test_predict_sieves_the_map_it_would_have_written(runs):
    f, raw = runs["f"], runs["raw"]
    got = _py("predict.py", "--ckpt", f("run.pt"), *PREDICT, "--sieve", "4", "--sieve_conn", "8", "--sieve_passes", "3", "--reliability",
              "--out", f("lab.npy"), "--proba", f("q.npy"), "--confidence", f("c.npy"))
    assert _oa_tags(got) == [" OA_ens", " OA_ens_sv"] and _oa_tags(raw) == [" OA_ens"]
    results = lambda lines: [ln for ln in lines if ln.startswith(("Result:", " OA", "producerA", "AA")) or ln.startswith("[")]
    assert results(got)[:len(results(raw))] == results(raw)                 # the raw block is printed as it is without the flag
    assert not any("sieve" in ln or "_sv" in ln for ln in raw)              # and a run without the flags says nothing new
    assert [ln.split(":")[0] for ln in got if ln.startswith("Reliability")] == ["Reliability_ens"]       # none behind _sv
    at = lambda s: next(k for k, ln in enumerate(got) if ln.startswith(s))
    assert at("sieve:") < at("sieve time ==") < at(" OA_ens_sv")
    lab0, p, lab, q, c = (np.load(f(x)) for x in ("lab0.npy", "p.npy", "lab.npy", "q.npy", "c.npy"))
    ref = _line(got, lab0, 4, 8, 3)
    assert lab.dtype == np.int64 and np.array_equal(lab, ref["out"])        # --out: sieve() of the un-sieved --out
    assert q.tobytes() == p.tobytes()                                       # --proba: the stage in front; labels move, not probabilities
    assert c.dtype == np.float32 and np.array_equal(c.view(np.int32), p[np.arange(len(lab)), lab].view(np.int32))
    moved = lab != lab0
    assert moved.sum() == ref["stats"][:, 3].sum() and (c[moved] <= np.load(f("c0.npy"))[moved]).all()
    oa = 100 * (lab == scene_truth()).mean()
    assert [ln for ln in got if ln.startswith(" OA_ens_sv=")][0].startswith(" OA_ens_sv=%.2f," % oa)


def test_the_sieve_is_last_behind_every_other_stage_and_one_network_takes_it(runs):
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", "--net", "1", "--tta", "2", "--smooth", "2", "--temperature", "2",
              "--sieve", "6", "--out", f("lab1.npy"))
    assert _oa_tags(got) == [" OA_tta", " OA_tta_smooth", " OA_tta_smooth_T", " OA_tta_smooth_T_sv"]
    at = lambda s: next(k for k, ln in enumerate(got) if ln.startswith(s))
    assert at("tempering time ==") < at("sieve:") < at("sieve time ==")
    assert np.load(f("lab1.npy")).dtype == np.int64


def test_sp_connect_votes_on_the_connected_map(runs, scene):  # noqa: F811
    f, ref = runs["f"], scene["ref"]
    got = _py("predict.py", "--ckpt", f("run.pt"), *PREDICT, "--superpixel", "4", "--sp_connect", "--save_segments", f("seg.npy"),
              "--out", f("labc.npy"))
    assert _oa_tags(got) == [" OA_ens", " OA_ens_sp"]
    ids, M = connect_segments_host(ref["seg"], ROWS, COLS, 4, 4, 4)
    before = cc_label_host(ref["seg"], ROWS, COLS, 4)["M"]
    line = [CONNECT.match(ln) for ln in got if ln.startswith("superpixel connectivity:")]
    assert len(line) == 1 and line[0] is not None and tuple(int(v) for v in line[0].groups()) == (before, before - M, M)
    stats = [ln for ln in got if ln.startswith("superpixel:")]
    counts = np.bincount(ids, minlength=M)
    assert len(stats) == 1 and stats[0].startswith("superpixel: segments=%d empty=0 mean_size=%.1f max_size=%d ASA=" % (
        M, counts.sum() / M, counts.max()))
    assert got.index(stats[0]) + 1 == got.index(line[0].group(0))           # the second line follows the first
    seg = np.load(f("seg.npy"))
    assert seg.dtype == np.int32 and np.array_equal(seg, ids)
    lab = np.load(f("labc.npy"))
    first = np.unique(seg, return_index=True)[1]
    assert np.array_equal(lab, lab[first][seg])                             # one label per connected segment
    assert not any("connectivity" in ln for ln in runs["raw"])


def test_what_the_command_lines_refuse(runs):
    f = runs["f"]
    r = _py("predict.py", "--ckpt", f("run.pt"), *PREDICT, "--sieve", "4", "--entropy", f("e.npy"), ok=False)
    assert r.returncode != 0 and "--entropy together with --sieve" in r.stderr and "moves labels, not probabilities" in r.stderr
    assert not os.path.exists(f("e.npy"))
    # (every other refusal is held in-process by tests/test_regions_host.py: each of these starts an interpreter)
    r = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", "--net", "both", "--sieve", "4", ok=False)
    assert r.returncode != 0 and "--net both" in r.stderr, r.stderr[-500:]
