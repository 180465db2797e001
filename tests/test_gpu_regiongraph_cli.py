"""GPU: the region-graph flags of the drivers (train.py / predict.py --superpixel S --region_graph) on the synthetic B2 scene,
one epoch, from a checkpoint made here.  What the drivers write is the library call's map (cmlpl_amd.regiongraph) of the same
networks on the same scene, byte for byte."""
import os
import re

import numpy as np
import pytest
import torch

from cmlpl_amd.regiongraph import RegionGraph, region_graph, region_propagate
from tests.gpu_util import DEV
from tests.test_gpu_superpixel_cli import COLS, ROWS, RUN, _oa_tags, _py, _timeless

pytestmark = pytest.mark.gpu
LINE = re.compile(r"^region graph: nodes=(\d+) knn=(\d+) adj=(\d+) edges=(\d+) max_in_degree=(\d+) truncated=(\d+) unreached=(\d+) "
                  r"residual=(\S+)$")
PREDICT = ["--synthetic", "B2", "--net", "ensemble"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rg"))
    f = lambda name: os.path.join(d, name)
    # (a checkpoint records the run's command line, paths included: both runs write the SAME paths, one after the other)
    files = ["--save_loss_hist", f("hist.npy"), "--save_ckpt", f("run.pt")]
    plain = _py("train.py", *RUN, *files)
    for name in ("hist.npy", "run.pt"):
        os.replace(f(name), f("plain_" + name))
    with_rg = _py("train.py", *RUN, "--superpixel", "4", "--region_graph", *files)
    raw = _py("predict.py", "--ckpt", f("run.pt"), *PREDICT, "--out", f("lab0.npy"), "--proba", f("p.npy"))
    return dict(with_rg=with_rg, plain=plain, raw=raw, f=f)


def _library(ckpt, probs, cfg, connect=False):
    """the library call on the checkpoint's two networks: (RegionGraphResult, RegionPropagated, the vote)"""
    import train
    from cmlpl_amd import checkpoint
    from cmlpl_amd.superpixel import Superpixel, superpixel_probs
    from hsi_loader import SyntheticScene
    ck = checkpoint.load(ckpt)
    shape = train.SYNTH["B2"]
    source = SyntheticScene(shape, ROWS, COLS, seed=3).cube_source(torch.device(DEV))
    models = train.build_nets(shape, [(0, ck["Base"]), (1, ck["Base1"])], torch.device(DEV), ck["identity"]["hp"]["dropout"])
    for m in models:
        m.eval()
    with torch.no_grad():
        vote = superpixel_probs(torch.from_numpy(probs).to(DEV), source.cube, Superpixel(4, connect=connect))
        ids, M = (vote.segments.seg, vote.segments.N) if not connect else (vote.connected, vote.M)
        rg = region_graph(ids, M, ROWS, COLS, source.spectra, models, cfg)
        return rg, region_propagate(rg, vote.seg_probs, cfg, conf=True, entropy=True), vote


def _line(lines, rg, out, cfg):
    got = [LINE.match(ln) for ln in lines if ln.startswith("region graph:")]
    assert len(got) == 1 and got[0] is not None, [ln for ln in lines if ln.startswith("region graph")]
    want = (rg.M, cfg.k, cfg.adj, rg.graph.edges(), rg.graph.max_in_degree(), int((rg.adjacency.deg > cfg.adj).sum()),
            int((out.regions.labels < 0).sum()))
    assert tuple(int(v) for v in got[0].groups()[:7]) == want
    assert got[0].group(8) == "%.3e" % float(out.regions.residual.cpu()[0])


def scene_truth():
    import train
    from hsi_loader import SyntheticScene
    return SyntheticScene(train.SYNTH["B2"], ROWS, COLS, seed=3).Y.numpy()


def test_train_adds_exactly_one_block_and_leaves_the_run_alone(runs):
    out, plain, f = runs["with_rg"], runs["plain"], runs["f"]
    assert _oa_tags(out) == [" OA", " OA1", " OA_ens_sp", " OA_ens_sp_rg"] and _oa_tags(plain) == [" OA", " OA1"]
    assert sum(ln.startswith("producerA_ens_sp_rg:") for ln in out) == 1 and sum(ln.startswith("AA_ens_sp_rg=") for ln in out) == 1
    assert sum("region graph time ==" in ln and "8 kNN + 8 adjacent" in ln for ln in out) == 1
    assert np.load(f("hist.npy")).tobytes() == np.load(f("plain_hist.npy")).tobytes()         # loss_hist bit-equal
    assert open(f("run.pt"), "rb").read() == open(f("plain_run.pt"), "rb").read()              # the checkpoint, every byte
    assert not any("region graph" in ln or "_rg" in ln for ln in plain)
    i = next(k for k, ln in enumerate(out) if ln.startswith("ensemble inference time"))
    assert _timeless(out[:i]) == _timeless(plain)                                              # every other line as it was
    at = lambda s: next(k for k, ln in enumerate(out) if ln.startswith(s))
    assert at("superpixel time ==") < at(" OA_ens_sp=") < at("region graph:") < at("region graph time ==") < at(" OA_ens_sp_rg=")
    rg, lib, _ = _library(f("run.pt"), np.load(f("p.npy")), RegionGraph())                     # the same networks, the same scene
    _line(out, rg, lib, RegionGraph())
    oa = 100 * (lib.labels.cpu().numpy() == scene_truth()).mean()
    assert [ln for ln in out if ln.startswith(" OA_ens_sp_rg=")][0].startswith(" OA_ens_sp_rg=%.2f," % oa)


def test_predict_writes_the_library_calls_map(runs):
    f, raw = runs["f"], runs["raw"]
    cfg = RegionGraph(k=4, adj=6, alpha=0.7, iters=30, net=1)
    got = _py("predict.py", "--ckpt", f("run.pt"), *PREDICT, "--superpixel", "4", "--region_graph", "--rg_k", "4", "--rg_adj", "6",
              "--rg_alpha", "0.7", "--rg_iters", "30", "--rg_net", "1", "--reliability", "--out", f("lab.npy"), "--proba", f("q.npy"),
              "--confidence", f("c.npy"), "--entropy", f("e.npy"))
    assert _oa_tags(got) == [" OA_ens", " OA_ens_sp", " OA_ens_sp_rg"] and _oa_tags(raw) == [" OA_ens"]
    results = lambda lines: [ln for ln in lines if ln.startswith(("Result:", " OA", "producerA", "AA")) or ln.startswith("[")]
    assert results(got)[:len(results(raw))] == results(raw)                 # the raw block is printed as it is without the flags
    assert not any("region graph" in ln or "_rg" in ln for ln in raw)       # and a run without the flags says nothing new
    assert [ln.split(":")[0] for ln in got if ln.startswith("Reliability")] == ["Reliability_ens", "Reliability_ens_sp", "Reliability_ens_sp_rg"]
    at = lambda s: next(k for k, ln in enumerate(got) if ln.startswith(s))
    assert at(" OA_ens_sp=") < at("region graph:") < at("region graph time ==") < at(" OA_ens_sp_rg=") < at("Reliability_ens_sp_rg")
    assert sum("region graph time ==" in ln and "member 1, 4 kNN + 6 adjacent" in ln for ln in got) == 1
    rg, lib, _ = _library(f("run.pt"), np.load(f("p.npy")), cfg)
    _line(got, rg, lib, cfg)
    lab, q, c, e = (np.load(f(x)) for x in ("lab.npy", "q.npy", "c.npy", "e.npy"))
    assert lab.dtype == np.int64 and np.array_equal(lab, lib.labels.cpu().numpy())             # --out: the library call's map
    for got_arr, want in ((q, lib.probs), (c, lib.conf), (e, lib.entropy)):                    # the last stage's, as ever
        assert got_arr.dtype == np.float32 and got_arr.tobytes() == want.cpu().numpy().tobytes()
    seg = rg.ids.cpu().numpy()
    first = np.unique(seg, return_index=True)[1]
    assert np.array_equal(lab, lab[first][seg])                                                # one label per region
    oa = 100 * (lab == scene_truth()).mean()
    assert [ln for ln in got if ln.startswith(" OA_ens_sp_rg=")][0].startswith(" OA_ens_sp_rg=%.2f," % oa)


def test_the_tags_compose(runs):
    f = runs["f"]
    got = _py("predict.py", "--ckpt", f("run.pt"), *PREDICT, "--smooth", "2", "--superpixel", "4", "--sp_connect", "--region_graph",
              "--sieve", "4", "--out", f("labc.npy"))
    assert _oa_tags(got) == [" OA_ens", " OA_ens_smooth", " OA_ens_smooth_sp", " OA_ens_smooth_sp_rg", " OA_ens_smooth_sp_rg_sv"]
    at = lambda s: next(k for k, ln in enumerate(got) if ln.startswith(s))
    assert at("superpixel connectivity:") < at("region graph:") < at("region graph time ==") < at("sieve:")
    nodes = int(LINE.match(got[at("region graph:")]).group(1))
    segments = int(re.search(r"segments=(\d+)$", got[at("superpixel connectivity:")]).group(1))
    assert nodes == segments                                                                   # the nodes are the connected map's
    assert np.load(f("labc.npy")).dtype == np.int64


def test_what_the_command_lines_refuse(runs):
    f = runs["f"]
    # (every other refusal is held in-process by tests/test_regiongraph_host.py: each of these starts an interpreter)
    r = _py("predict.py", "--ckpt", f("run.pt"), *PREDICT, "--region_graph", "--out", f("no.npy"), ok=False)
    assert r.returncode != 0 and "--region_graph belongs to --superpixel" in r.stderr, r.stderr[-500:]
    r = _py("predict.py", "--ckpt", f("run.pt"), "--synthetic", "B2", "--net", "both", "--superpixel", "4", "--region_graph", ok=False)
    assert r.returncode != 0 and "--region_graph gives ONE prediction" in r.stderr and "--net both" in r.stderr, r.stderr[-500:]
    r = _py("train.py", *RUN, "--superpixel", "4", "--region_graph", "--rg_k", "20", "--rg_adj", "13", ok=False)
    assert r.returncode != 0 and "k + adj 1 .. 32" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(f("no.npy"))
