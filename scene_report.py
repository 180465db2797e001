"""Whole-scene prediction and its report, under ``train.py`` (the end of a run) and ``predict.py``: one scene record
(``SceneJob``), a first prediction (``ensemble_first`` / ``tta_first``), the stages behind it (``smooth_stage``,
``superpixel_stage``, ``region_graph_stage``, ``temper_stage``, ``sieve_stage``) and one runner (``run_scene``: the scene opened, then ``run_stages``), which owns the
tags of the ``Result:`` blocks, what every step hands on and what becomes of the first block; ``evaluate_whole`` beside it."""
import time
from collections import namedtuple
from typing import Any, NamedTuple, Optional

import numpy as np
import torch

from cmlpl_amd import NetShape
from tools.hyper_tools import CalAccuracy, test_whole
from tools.models import BaseNet2

NET_TAGS = {0: '', 1: '1', 'ema0': '_ema', 'ema1': '_ema1',      # evaluate_whole: a network, or a network's EMA teacher
            'ens': '_ens',                                         # ensemble_first: several of them together
            'tta': '_tta'}                                         # tta_first: over noisy views of every pixel
SMOOTH_TAG = '_smooth'                                             # smooth_stage: appended to the tag of what it smooths
SP_TAG = '_sp'                                                     # superpixel_stage: appended to the tag of what votes
RG_TAG = '_rg'                                                     # region_graph_stage: appended to the tag of the vote it diffuses
TEMPER_TAG = '_T'                                                  # temper_stage: appended to the tag of what it tempers
SIEVE_TAG = '_sv'                                                  # sieve_stage: appended to the tag of the map it sieves
PRINT, SCORE, SILENT = 'print', 'score', 'silent'                  # run_stages: what happens to the first prediction's block
OUTPUTS = ("labels", "probs", "conf", "entropy")                   # the leading fields of every result tuple


class SceneJob(NamedTuple):
    """the scene of a report: the networks' ``shape`` (C, H, W, bands, K), ``whole`` the dataset (or SyntheticScene), the labelled
    test pixels and their classes (None: no ``Result:`` lines), ``resident_cube`` the scene already on the device (a cube-fed run's)"""
    shape: tuple
    whole: Any
    device: Any
    synthetic: Optional[str] = None
    dataID: int = 1
    dropout: float = 0.8
    test_array: Any = None
    Y_test: Any = None
    resident_cube: Any = None


# the first prediction: ``predict(models, cube, spectra, want)`` is the library call, ``timing`` its printed line (a format of the
# seconds and the number of networks), ``tag`` that of its ``Result:`` lines, ``noun`` who asks for the scene cube.  A further stage:
# ``call(result, cube, want)`` on the result in front of it, ``timing`` a format of the seconds, ``suffix`` what its lines append
# to the running tag, ``noun`` as above (None: nobody new asks), ``scored`` False: its probabilities are those of the stage in front
# -- it moves labels only --, so ``score`` is not called behind its block; ``scene`` True: ``call(result, cube, want, spectra,
# models)`` -- the stage also reads the scene's spectra and the member models
First = namedtuple('First', 'predict timing tag noun', defaults=("the ensemble",))
Stage = namedtuple('Stage', 'timing suffix call noun scored scene', defaults=(None, True, False))
SieveOut = namedtuple('SieveOut', 'labels probs conf entropy stats')


def tta_tag(tta):
    """the tag of a TTA prediction's ``Result:`` lines: ``_tta``, with ``_flips`` / ``_d4`` behind it when its views are spatial"""
    return NET_TAGS['tta'] + ('' if tta.spatial == 'none' else '_' + tta.spatial)


def tta_timing(tta):
    """the timing line of a TTA prediction (a format of the seconds and the number of networks)"""
    return 'tta inference time == %%.3f s (%%d networks x %d views%s, noise %g%s)' % (
        tta.views, ' + the clean window' if tta.clean else '', tta.sigma,
        '' if tta.spatial == 'none' else ', spatial ' + tta.spatial)


def print_block(tag, OA, Kappa, producerA, AA):
    """the ``Result:`` / ``producerA`` / ``AA`` lines (train.py:297-306) of fractions, in per cent"""
    print('Result:\n OA%s=%.2f,Kappa=%.2f' % (tag, OA * 100, Kappa * 100))
    print('producerA%s:' % tag, producerA * 100)
    print('AA%s=%.2f' % (tag, AA * 100))


def print_result(tag, pred, rows, truth):
    """the block of one label map scored on its positions ``rows`` against ``truth``; returns its OA"""
    OA, Kappa, producerA = CalAccuracy(pred[rows], truth)
    print_block(tag, OA, Kappa, producerA, np.mean(producerA))
    return OA


def scene_source(job):
    """the scene as a ``CubeSource`` for the cube-fed forward, or None: a window shape the per-sample forward does not
    take, or a dataset directory without its cube"""
    from cmlpl_amd.infer import infer_supported
    if not infer_supported(NetShape(*job.shape)):
        return None
    if job.synthetic:  # (a SyntheticScene is its own scene; a directory without scene.json looks its scene up by dataID)
        return job.whole.cube_source(job.device, resident_cube=job.resident_cube)
    return job.whole.cube_source(job.device, dataID=job.dataID, resident_cube=job.resident_cube)


def build_nets(shape, nets, device, dropout):
    """the ``BaseNet2`` modules of ``nets`` = [(key, state_dict)], on ``device``, in that order"""
    models = [BaseNet2(num_features=shape[3], dropout=dropout, num_classes=shape[4], in_channels=shape[0],
                       window=shape[1]).to(device) for _ in nets]
    for model, (_, sd) in zip(models, nets):
        model.load_state_dict(sd)
    return models


class RelScore:
    """``--reliability``: the ``Reliability<tag>:`` line behind a ``Result:`` block -- the reliability counters of the block's
    class probabilities at the positions ``rows`` against ``truth`` (cmlpl_amd.calibrate.reliability: one launch, one read-back).
    ``held_out``: positions in ``rows`` the lines are counted on (the rest fitted a temperature); the line says so.
    ``blocks`` keeps the int64 counter block of every line, by tag."""

    def __init__(self, rows, truth, device, bins=15, held_out=None):
        rows, truth = np.asarray(rows, np.int64), np.asarray(truth, np.int64)
        self.note = ''
        if held_out is not None:
            rows, truth = rows[held_out], truth[held_out]
            self.note = ' (held-out n=%d)' % len(rows)
        self.rows, self.truth = (torch.from_numpy(np.ascontiguousarray(v)).to(device) for v in (rows, truth))
        self.bins, self.blocks = bins, {}

    def __call__(self, tag, res):
        from cmlpl_amd.calibrate import reliability
        rel = reliability(res.probs, self.truth, self.rows, self.bins)
        self.blocks[tag] = rel.counts
        print(rel.line(tag, self.note))

    def save(self, path):
        np.savez(path, **{'Reliability' + tag: block for tag, block in self.blocks.items()})


def calibration_split(n, frac, seed):
    """(calibration, held-out) positions among n labelled test pixels: a seeded random share ``frac`` fits the temperature
    (the first round(frac n) of numpy.random.default_rng(seed).permutation(n)), the remainder scores it"""
    perm = np.random.default_rng(seed).permutation(n)
    k = int(round(frac * n))
    return perm[:k], perm[k:]


def ensemble_first(tag=NET_TAGS['ens']):
    """the first prediction of 1..4 networks TOGETHER: the label of their averaged softmax for every scene pixel
    (cmlpl_amd.ensemble.ensemble_cube: every member's eval forward from the resident cube, one launch behind each chunk);
    ``tag``: a single network's own, where its softmax is a one-member ensemble behind its ``evaluate_whole`` block"""
    from cmlpl_amd.ensemble import ensemble_cube
    return First(lambda models, cube, spectra, want: ensemble_cube(models, cube, spectra, **want),
                 'ensemble inference time == %.3f s (%d networks)', tag)


def tta_first(tta):
    """the first prediction over the views of ``tta`` (cmlpl_amd.tta.TTA): every network scores every view of every scene
    pixel, one label map from the average of all their softmaxes (cmlpl_amd.tta.tta_cube)"""
    from cmlpl_amd.tta import tta_cube
    return First(lambda models, cube, spectra, want: tta_cube(models, cube, spectra, tta, **want),
                 tta_timing(tta), tta_tag(tta), "test-time augmentation")


def stage_want(want):
    """a stage's output keywords: what ``ensemble_cube`` calls ``probs`` the stages call ``probs_out``"""
    return dict(probs_out=want['probs'], conf=want['conf'], entropy=want['entropy'])


def smooth_stage(smooth):
    """the stage that smooths the probabilities in front of it under the guide of the scene cube (``smooth``: a
    cmlpl_amd.smooth.Smooth; cmlpl_amd.smooth.smooth_probs)"""
    from cmlpl_amd.smooth import smooth_probs
    R, ss, sr, G, iters = smooth.params()
    return Stage('smoothing time == %%.3f s (radius %d, sigma_s %g, sigma_r %g, up to %d guide channels, %d pass%s)' %
                 (R, ss, sr, G, iters, '' if iters == 1 else 'es'), SMOOTH_TAG,
                 lambda res, cube, want: smooth_probs(res.probs, cube, smooth, **stage_want(want)), "spatial smoothing")


def superpixel_stage(sp, job, save_segments=None):
    """the stage in which the regions vote (``sp``: a cmlpl_amd.superpixel.Superpixel; cmlpl_amd.superpixel.superpixel_probs):
    the scene is segmented, every superpixel votes with the probabilities (``--sp_vote hard``: the labels) in front of it, and
    one line ``superpixel: segments= empty= mean_size= max_size= ASA=`` says what the map is (ASA on ``job``'s labelled test
    pixels: the accuracy no region-level labelling of this map can exceed).  ``save_segments``: the int32 segment map's file."""
    from cmlpl_amd.superpixel import asa, superpixel_probs
    S, m, T, G, vote = sp.params()

    def call(res, cube, want):
        out = superpixel_probs(res.probs, cube, sp, labels=res.labels, **stage_want(want))
        segs = out.segments
        if out.connected is None:
            seg, N, counts = segs.seg, segs.N, segs.counts.cpu().numpy()
        else:           # --sp_connect: the line describes the connected map, the one that voted (the segmenter's counts are of regular pixels)
            seg, N, counts = out.connected, out.M, torch.bincount(out.connected.long(), minlength=out.M).cpu().numpy()
        bound = 'n/a' if job.test_array is None else '%.4f' % asa(seg, N, job.test_array, job.Y_test, job.shape[4])
        print('superpixel: segments=%d empty=%d mean_size=%.1f max_size=%d ASA=%s' %
              (N, int((counts == 0).sum()), counts.sum() / N, counts.max(), bound))
        if out.connected is not None:
            from cmlpl_amd.regions import components
            before = components(segs.seg, cube.shape[0], cube.shape[1]).count()
            print('superpixel connectivity: components_before=%d fragments_merged=%d segments=%d' % (before, before - N, N))
        if save_segments:
            np.save(save_segments, seg.cpu().numpy())
        return out
    return Stage('superpixel time == %%.3f s (step %d, compactness %g, %d iterations, up to %d guide channels, %s vote%s)' %
                 (S, m, T, G, vote, ', connected' if sp.connect else ''), SP_TAG, call, "the superpixel vote")


def region_graph_stage(cfg):
    """the stage DIRECTLY behind the superpixel stage: the regions that voted become the nodes of a label propagation
    (``cfg``: a cmlpl_amd.regiongraph.RegionGraph; region_graph + region_propagate) -- every region is described by the
    embedding of its mean spectrum under member ``cfg.net``, linked to its most similar and to its adjacent regions, and the
    vote's probabilities are the prior that diffuses.  One line ``region graph: nodes= knn= adj= edges= max_in_degree=
    truncated= unreached= residual=`` (truncated: regions that touch more than ``adj`` others)."""
    from cmlpl_amd.regiongraph import region_graph, region_propagate
    cfg = cfg.check()

    def call(res, cube, want, spectra, models):
        if getattr(res, 'seg_probs', None) is None or getattr(res, 'segments', None) is None:
            raise SystemExit("the region graph stands directly behind the superpixel vote")
        rows, cols = cube.shape[0], cube.shape[1]
        ids, M = (res.segments.seg, res.segments.N) if res.connected is None else (res.connected, res.M)
        rg = region_graph(ids, M, rows, cols, spectra, list(models), cfg)
        out = region_propagate(rg, res.seg_probs, cfg, **stage_want(want))
        print('region graph: nodes=%d knn=%d adj=%d edges=%d max_in_degree=%d truncated=%d unreached=%d residual=%.3e' %
              (M, cfg.k, cfg.adj, rg.graph.edges(), rg.graph.max_in_degree(), int((rg.adjacency.deg > cfg.adj).sum()),
               int((out.regions.labels < 0).sum()), float(out.regions.residual.cpu()[0])))
        return out
    return Stage('region graph time == %%.3f s (member %d, %d kNN + %d adjacent neighbours, alpha %g, gamma %d, %d iterations)' %
                 (cfg.net, cfg.k, cfg.adj, cfg.alpha, cfg.gamma, cfg.iters), RG_TAG, call, "the region graph", True, True)


def temper_stage(T, fit=None):
    """the stage that tempers the probabilities in front of it (cmlpl_amd.calibrate.temper_probs).  ``T`` None: fitted first,
    on the pixels ``fit`` = (rows, truth) on the device"""
    from cmlpl_amd.calibrate import fit_temperature, temper_probs

    def call(res, cube, want):
        t = T
        if t is None:
            t, before, after = fit_temperature(res.probs, fit[1], fit[0])
            print('temperature = %.4f (NLL %.4f -> %.4f on the calibration share)' % (t, before, after))
        return temper_probs(res.probs, t, **stage_want(want))
    return Stage('tempering time == %%.3f s (T %s)' % ('fitted' if T is None else '%g' % T), TEMPER_TAG, call)


def sieve_stage(sv):
    """the LAST stage: connected regions of fewer than ``min_size`` pixels of the label map in front take the label of the
    largest large region they touch (``sv``: a cmlpl_amd.regions.Sieve; cmlpl_amd.regions.sieve).  One line ``sieve: components=
    small= relabelled= passes_used= components_after=`` from the counters of its passes.  It moves labels, never probabilities:
    ``probs`` are those of the stage in front, ``conf`` is every pixel's own probability of the label it ends with, there is no
    entropy of its own, and no ``Reliability`` line behind its block."""
    from cmlpl_amd.regions import components, sieve
    min_size, conn, passes = sv.params()

    def call(res, cube, want):
        rows, cols = cube.shape[0], cube.shape[1]
        out = sieve(res.labels.contiguous(), rows, cols, sv, probs=res.probs if want.get('conf') else None)
        s = out.summary()
        if s['components_after'] is None:       # (the last pass still moved pixels: its counters do not say what it left)
            s['components_after'] = components(out.labels.to(torch.int32), rows, cols, conn).count()
        print('sieve: components=%(components)d small=%(small)d relabelled=%(relabelled)d passes_used=%(passes_used)d '
              'components_after=%(components_after)d' % s)
        return SieveOut(out.labels, res.probs if want.get('probs') else None, out.conf, None, out.stats)
    return Stage('sieve time == %%.3f s (min_size %d, %d-connected, up to %d pass%s)' %
                 (min_size, conn, passes, '' if passes == 1 else 'es'), SIEVE_TAG, call, "the sieve", False)


def run_stages(first, stages, cube, spectra, models, job, first_block=PRINT, want=None, score=None):
    """``first`` = (predict, timing, tag), then ``stages`` = [(timing, suffix, call), ..], each on the result in front of it
    (a ``Stage`` with ``scene`` also takes the spectra and the models).
    Per step: the library call, the copy to the host, the timing line, the ``Result:`` block (when ``job`` has the test pixels)
    under the RUNNING tag -- ``first``'s, plus the suffix of every stage so far --, then ``score(tag, result)`` (a ``RelScore``; not behind a stage that is not ``scored``).
    ``want`` (probs / conf / entropy: the caller's wishes) goes to the LAST step; every step in front of it is asked for its
    probabilities and nothing else, and with a ``score`` every step produces them.  ``first_block``: PRINT the first block and
    score it, SCORE it only (``evaluate_whole`` printed it), or SILENT.  Returns the last step's outputs as numpy arrays, by
    name; what it did not produce is absent."""
    predict, timing, tag = first[:3]
    want = dict(want or {}, **(dict(probs=True) if score is not None else {}))
    asked = [{k: bool(w.get(k)) for k in OUTPUTS[1:]} for w in [dict(probs=True)] * len(stages) + [want]]
    steps = [(timing, '', lambda res, cube, ask: predict(models, cube, spectra, ask)), *stages]
    res = None
    for i, ((timing, suffix, call, *more), ask) in enumerate(zip(steps, asked)):
        tag += suffix
        t1 = time.time()
        res = call(res, cube, ask, spectra, models) if len(more) > 2 and more[2] else call(res, cube, ask)
        out = {k: v.cpu().numpy() for k, v in zip(OUTPUTS, res[:4]) if v is not None}
        print(timing % ((time.time() - t1, len(models)) if i == 0 else time.time() - t1))
        if job.test_array is not None and (i > 0 or first_block == PRINT):
            print_result(tag, out["labels"], job.test_array, job.Y_test)
        if score is not None and (i > 0 or first_block != SILENT) and (len(more) < 2 or more[1]):
            score(tag, res)
    return out


def run_scene(job, nets, first, stages=(), **how):
    """``run_stages`` of ``nets`` = [(key, state_dict)] on the opened scene, which the stages need as its cube (there is no
    loader fall-back); who asks for it is the last stage with a noun, else the first prediction"""
    source = scene_source(job)
    if source is None:
        raise SystemExit("%s needs the scene cube (cube.npy + scene.json in the dataset directory, sample_generation.py) and a "
                         "square window" % next((stage.noun for stage in reversed(stages) if stage.noun), first.noun))
    models = [model.eval() for model in build_nets(job.shape, nets, job.device, job.dropout)]
    return run_stages(first, stages, source.cube, source.spectra, models, job, **how)


def evaluate_whole(job, nets, val_batch_size=512, last_eval=None):
    """Whole-image inference + accuracy (train.py:291-306) of ``nets`` = [(network index -- or 'ema0' / 'ema1', a network's
    EMA teacher --, state_dict)]: the end of a training run, and all of predict.py.  Returns {network index: int64 label per scene pixel}.
    The scene stays in HBM as its cube and the forward gathers the windows itself (cmlpl_infer_cube): no 19.9 GB patch
    tensor, no DataLoader (train.py:291-294 streams the materialised patches).  Window shapes the per-sample forward does
    not take, or a dataset directory without the cube, fall back to the loader.  The source is built ONCE for all
    networks, and its load time is printed (the reference's "inference time" includes streaming the data).  The ``Result:``
    lines need ``job``'s test pixels.  ``last_eval``: the [net][OA, AA, Kappa] row of --eval_every when it scored these parameters."""
    shape, whole, device = job.shape, job.whole, job.device
    t_src = time.time()
    source = scene_source(job)
    if source is None:
        if job.synthetic:  # (cut the scene's windows on the device, then the reference's loader path)
            from cmlpl_amd.patches import extract_patches
            XPw = extract_patches(whole.cube_source(device).cube, torch.arange(len(whole), device=device), shape[1]).cpu()
            source = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(XPw, whole.X),
                                                 batch_size=val_batch_size, shuffle=False)
        else:
            source = torch.utils.data.DataLoader(whole, batch_size=val_batch_size, shuffle=False)
    if device.type == "cuda":
        torch.cuda.synchronize()
    print('evaluation source ready in %.3f s' % (time.time() - t_src))
    preds = {}
    for (net, _), model in zip(nets, build_nets(shape, nets, device, job.dropout)):  # (test_whole sets .eval() itself)
        t1 = time.time()
        pred = preds[net] = test_whole(model, source, print_per_batches=10 ** 9)
        print('inference time == %.3f s' % (time.time() - t1))
        if job.test_array is None:
            continue
        tag = NET_TAGS[net]
        OA = print_result(tag, pred, job.test_array, job.Y_test)
        if last_eval is not None and net in (0, 1):
            # the last epoch was scored by --eval_every too: both are exact counts on the same pixels
            same = last_eval[net][0] == OA
            print('validation check%s: matrix OA %s whole-image OA (%.6f / %.6f)' %
                  (tag, '==' if same else '!=', last_eval[net][0] * 100, OA * 100))
    return preds
