#!/usr/bin/env python3
"""Classify a scene with a trained pair of networks: the third stage after ``sample_generation.py`` and ``train.py``.

    python train.py --dataID 1 --save_ckpt run.ckpt
    python predict.py --ckpt run.ckpt --dataID 1 --out labels.npy

The window shape and the class count come from the checkpoint (cmlpl_amd.checkpoint); the scene is the dataset
directory's ``cube.npy`` + ``scene.json`` (``HSIDataSet(.., 'wholeset').cube_source``), labelled on the device by
``cmlpl_infer_cube`` through ``tools.hyper_tools.test_whole`` -- the end-of-run evaluation of ``train.py``
(``train.evaluate_whole``), without a training engine.  ``--out`` receives the int64 label map [rows * cols]
(``--net both``: [2][rows * cols]; ``--net ema0 | ema1 | ema_both``: the EMA teachers of a ``train.py --ema`` run); when the directory has ``test_array.npy`` / ``Y.npy`` the ``Result:`` / ``producerA`` /
``AA`` lines of ``train.py`` are printed.  ``--net ensemble`` labels the scene with Base and Base1 TOGETHER -- the first
maximum of their averaged softmax (cmlpl_amd.ensemble; ``ensemble_all`` adds both EMA teachers) -- and prints the lines
with the tag ``_ens``; ``--proba`` / ``--confidence`` / ``--entropy`` write the class probabilities float32
[rows * cols, K], the probability of the label and the entropy float32 [rows * cols] -- of the ensemble, or of a single
``--net`` (its own softmax: a one-member ensemble; its label map stays the argmax of its logits).  ``--synthetic SHAPE`` labels the seeded synthetic scene that
``train.py --synthetic`` evaluates on (datasets are not shipped).  ``--tta M`` predicts from the clean window and M noisy views
(x + S N(0,1), S = ``--tta_noise``, default the checkpoint's training noise) of every pixel, averaged over the views and
over the networks of ``--net`` (any single network or ensemble; cmlpl_amd.tta): the label map, the ``Result:`` lines (tag
``_tta``) and ``--proba`` / ``--confidence`` / ``--entropy`` then describe that prediction.  ``--tta_spatial flips | d4`` makes
the views flipped (and rotated) windows as well -- what ``train.py --aug_spatial`` trains on; ``--tta 7 --tta_noise 0
--tta_spatial d4`` is the plain orbit of the eight elements -- and the tag ``_tta_flips`` / ``_tta_d4``.  ``--smooth R`` smooths the class
probability maps of that prediction over the scene -- an edge-preserving filter of radius R guided by the cube's leading
channels (cmlpl_amd.smooth; ``--smooth_sigma_s`` / ``--smooth_sigma_r`` / ``--smooth_guide`` / ``--smooth_iters``), with any single
network or ensemble, with or without ``--tta``: the ``Result:`` block above is printed as it is, a second one follows with
``_smooth`` appended to its tag, and ``--out`` / ``--proba`` / ``--confidence`` / ``--entropy`` describe the SMOOTHED prediction.
``--reliability`` prints, behind every ``Result:`` block of ONE prediction (the raw one, ``_ens``, ``_tta..``, ``.._smooth``, ``.._T``),
one line ``Reliability<tag>: ECE=.. MCE=.. NLL=.. Brier=.. conf=.. acc=..`` over the labelled test pixels -- whether a written
confidence means what it says (cmlpl_amd.calibrate: integer counters on the device, ``--rel_bins`` bins, default 15;
``--save_reliability FILE`` writes the int64 blocks as .npz, one entry ``Reliability<tag>`` per line); for a single ``--net`` the
probabilities are its own softmax.  ``--temperature T`` tempers the FINAL probabilities of the prediction (behind TTA and
smoothing), ``q = softmax(log p / T)``: a further ``Result:`` block follows with ``_T`` appended to the tag, and ``--out`` /
``--proba`` / ``--confidence`` / ``--entropy`` describe the tempered prediction.  ``--temperature fit`` finds T itself, the least
NLL on a seeded random share (``--calib_frac``, default 0.5; ``--calib_seed``, default 1088) of the labelled test pixels; every
``Reliability`` line of such a run is counted on the held-out remainder only, and says so.  ``--knn K`` scores the EMBEDDING
instead of the classifier: the weighted kNN vote (cmlpl_amd.knn: K neighbours by cosine similarity of the spectral branch's
``feat``, weights exp(s / T), T = ``--knn_T``, default the checkpoint's training temperature) of the labelled test pixels over
the training pixels (``--knn_gallery train``) or leave-one-out among themselves (``loo``): one ``Result:`` block per network of
``--net 0 | 1 | both | ema0 | ema1 | ema_both`` with the tag ``_knn``, ``--reliability`` prints its line behind it (the vote's
probabilities are a probability map over the test list), ``--embed FILE`` writes the float32 [n_test][1024] embedding of a
single network.  No label map is written: the vote is over the test list, not the scene.  ``--propagate`` (``--lp_k`` / ``--lp_alpha`` /
``--lp_gamma`` / ``--lp_iters``; defaults 10, 0.99, 3, 50, not tuned) is the transductive second opinion on the same embedding: label
propagation over its kNN graph (cmlpl_amd.labelprop) -- the nodes are the labelled training pixels, which are the seeds (the
gallery of ``--knn_gallery train``), followed by the labelled test pixels.  Per network of ``--net`` one line ``propagate<tag>: nodes=..
edges=.. max_in_degree=.. unreached=.. residual=..`` and a ``Result:`` block with the tag ``_lp`` scored on the test pixels (one the seeds
do not reach counts as wrong); ``--reliability`` prints its line behind it.  With ``--knn`` both appear: ``_knn`` first, then ``_lp``.
``--superpixel S`` classifies REGIONS: the scene is over-segmented into superpixels on a grid of step S under the cube's leading
channels and every region votes with the class probabilities of its pixels (cmlpl_amd.superpixel; ``--sp_compact`` / ``--sp_iters`` /
``--sp_guide`` / ``--sp_vote soft | hard``), with any single network or ensemble, with or without ``--tta``, behind ``--smooth`` when
given and in front of ``--temperature``: one line ``superpixel: segments=.. empty=.. mean_size=.. max_size=.. ASA=..`` (ASA: the
accuracy on the labelled test pixels that no region-level labelling of this map can exceed), a further ``Result:`` block with
``_sp`` appended to the tag, and ``--out`` / ``--proba`` / ``--confidence`` / ``--entropy`` describe the last stage.  ``--save_segments
FILE`` writes the int32 segment map.  ``--sp_connect`` makes the regions that vote CONNECTED (fragments of fewer than S S / 4 pixels
join the largest region they touch, every remaining component is a segment of its own): the ``superpixel:`` line and
``--save_segments`` then describe that map, and a line ``superpixel connectivity: components_before=.. fragments_merged=..
segments=..`` follows.  ``--region_graph`` (``--rg_k K``, ``--rg_adj A``, ``--rg_alpha a``, ``--rg_gamma g``, ``--rg_iters T``,
``--rg_net i``; with ``--superpixel S``, directly behind it) makes the regions that voted the nodes of a label propagation: each is
described by the embedding of its mean spectrum under member i of --net, linked to its K most similar and its A adjacent regions,
and the vote is the prior that diffuses (cmlpl_amd.regiongraph): one line ``region graph: nodes=.. knn=.. adj=.. edges=..
max_in_degree=.. truncated=.. unreached=.. residual=..`` and a further ``Result:`` block with ``_rg`` appended to the tag.  ``--sieve N`` (``--sieve_conn 4 | 8``, ``--sieve_passes T``) sieves the label map, LAST in the chain -- behind
``--smooth``, ``--superpixel`` and ``--temperature``, which never moves a label: a connected region of fewer than N pixels takes the
label of the largest region of at least N pixels that it touches (cmlpl_amd.regions), with any single network or ensemble, with
or without ``--tta``.  One line ``sieve: components=.. small=.. relabelled=.. passes_used=.. components_after=..``, a further
``Result:`` block with ``_sv`` appended to the tag (no ``Reliability`` line: the sieve moves labels, not probabilities); ``--out`` is
the sieved map, ``--confidence`` the pixel's own probability of the label it ends with, ``--proba`` the probabilities of the stage
in front; ``--entropy`` is refused with ``--sieve``."""
import argparse
import os
from collections import namedtuple

import numpy as np
import torch

from cmlpl_amd import checkpoint
from cmlpl_amd.tta import TTA
from hsi_loader import HSIDataSet, SyntheticScene
from scene_report import (NET_TAGS, PRINT, SCORE, SILENT, RelScore, SceneJob, build_nets, calibration_split, ensemble_first,
                          evaluate_whole, print_block, print_result, region_graph_stage, run_scene, sieve_stage, smooth_stage, superpixel_stage,
                          temper_stage,
                          tta_first, tta_tag)
from train import (DATASETS, SPATIAL_MODES, SYNTH, add_propagate_flags, add_region_graph_flags, add_sieve_flags, add_smooth_flags, add_superpixel_flags,
                   on_device, propagate_nodes, propagate_of, region_graph_of, sieve_of, smooth_of, superpixel_of)

ENSEMBLES = {'ensemble': [0, 1], 'ensemble_all': [0, 1, 'ema0', 'ema1']}
CALIB_FRAC, CALIB_SEED, REL_BINS = 0.5, 1088, 15                 # the defaults of --calib_frac / --calib_seed / --rel_bins


def temperature_of(args):
    """--temperature: None (not given), 'fit', or a finite T > 0; anything else is a SystemExit"""
    t = getattr(args, 'temperature', None)
    if t is None or t == 'fit':
        return t
    try:
        t = float(t)
    except ValueError:
        t = float('nan')
    if not (0.0 < t < float('inf')):
        raise SystemExit("--temperature T: a finite T > 0, or 'fit'")
    return t


def check_args(args):
    """what the command line cannot mean, said before anything is loaded"""
    if args.net in ('both', 'ema_both') and (args.proba or args.confidence or args.entropy):
        raise SystemExit("--proba / --confidence / --entropy describe ONE prediction: --net %s writes two label maps "
                         "(name one network, or --net ensemble for the two together)" % args.net)
    if args.tta is not None:
        if args.net in ('both', 'ema_both'):
            raise SystemExit("--tta gives ONE prediction: --net %s writes two label maps (name one network, or --net "
                             "ensemble for the two together)" % args.net)
        if args.tta < 1 or args.tta > 63:
            raise SystemExit("--tta M: 1 .. 63 views")
        if args.tta_noise is not None and not (0.0 <= args.tta_noise < float("inf")):
            raise SystemExit("--tta_noise S: a finite S >= 0")
        if args.tta_seed < 0 or args.tta_seed >= 2 ** 64:
            raise SystemExit("--tta_seed N: 0 <= N < 2^64")
    elif args.tta_noise is not None or args.tta_no_clean or args.tta_spatial != 'none':
        raise SystemExit("--tta_noise / --tta_no_clean / --tta_spatial belong to --tta M")
    temperature = temperature_of(args)
    if args.net in ('both', 'ema_both') and (args.reliability or temperature is not None):
        raise SystemExit("--reliability / --temperature describe ONE prediction: --net %s writes two label maps (name one "
                         "network, or --net ensemble for the two together)" % args.net)
    if not args.reliability and (args.rel_bins is not None or args.save_reliability):
        raise SystemExit("--rel_bins / --save_reliability belong to --reliability")
    if args.rel_bins is not None and not 1 <= args.rel_bins <= 1024:
        raise SystemExit("--rel_bins B: 1 .. 1024 bins")
    if temperature != 'fit' and (args.calib_frac is not None or args.calib_seed is not None):
        raise SystemExit("--calib_frac / --calib_seed belong to --temperature fit")
    if args.calib_frac is not None and not (0.0 < args.calib_frac < 1.0):
        raise SystemExit("--calib_frac F: a share 0 < F < 1 of the labelled test pixels")
    if args.calib_seed is not None and args.calib_seed < 0:
        raise SystemExit("--calib_seed N: N >= 0")
    if smooth_of(args) is not None and args.net in ('both', 'ema_both'):
        raise SystemExit("--smooth gives ONE prediction: --net %s writes two label maps (name one network, or --net "
                         "ensemble for the two together)" % args.net)
    if getattr(args, 'region_graph', None) is not None and args.net in ('both', 'ema_both'):
        raise SystemExit("--region_graph gives ONE prediction: --net %s writes two label maps (name one network, or --net "
                         "ensemble for the two together)" % args.net)
    region_graph_of(args, len(networks_of(args)))
    if superpixel_of(args) is not None:
        if args.net in ('both', 'ema_both'):
            raise SystemExit("--superpixel gives ONE prediction: --net %s writes two label maps (name one network, or --net "
                             "ensemble for the two together)" % args.net)
        if args.knn is not None or args.embed or getattr(args, 'propagate', False):
            raise SystemExit("--superpixel votes over the scene's map: --knn / --embed / --propagate describe the labelled test "
                             "pixels, a list without a map")
    if sieve_of(args) is not None:
        if args.entropy:
            raise SystemExit("--entropy together with --sieve: the sieve moves labels, not probabilities, so the sieved map has no "
                             "entropy of its own (write --entropy without --sieve, or --confidence, the pixel's own probability of "
                             "the label it ends with)")
        if args.net in ('both', 'ema_both'):
            raise SystemExit("--sieve gives ONE prediction: --net %s writes two label maps (name one network, or --net "
                             "ensemble for the two together)" % args.net)
        if args.knn is not None or args.embed or getattr(args, 'propagate', False):
            raise SystemExit("--sieve works on the scene's map: --knn / --embed / --propagate describe the labelled test pixels, a "
                             "list without a map")


def check_knn_args(args):
    """what --knn / --embed cannot mean"""
    if args.knn is None:
        if args.knn_T is not None or args.knn_gallery is not None:
            raise SystemExit("--knn_T / --knn_gallery belong to --knn K")
        if args.embed is None:
            return
    elif not 1 <= args.knn <= 32:
        raise SystemExit("--knn K: 1 .. 32 neighbours")
    if args.knn_T is not None and not (0.0 < args.knn_T < float("inf")):
        raise SystemExit("--knn_T T: a finite T > 0")
    if args.net in ENSEMBLES:
        raise SystemExit("--knn / --embed score the embedding of ONE network at a time: --net %s averages class probabilities "
                         "(name a network, or both / ema_both)" % args.net)
    if args.embed and args.net in ('both', 'ema_both'):
        raise SystemExit("--embed writes the embedding of a single network: not with --net %s" % args.net)
    if args.out or args.proba or args.confidence or args.entropy or args.tta is not None or smooth_of(args) is not None \
            or temperature_of(args) is not None:
        raise SystemExit("--knn / --embed describe the labelled test pixels, not the scene: not with --out, --proba, --confidence, "
                         "--entropy, --tta, --smooth or --temperature")


def check_propagate_args(args):
    """what --propagate cannot mean (the refusals of --knn)"""
    if propagate_of(args) is None:
        return
    if args.net in ENSEMBLES:
        raise SystemExit("--propagate scores the embedding of ONE network at a time: --net %s averages class probabilities "
                         "(name a network, or both / ema_both)" % args.net)
    if args.out or args.proba or args.confidence or args.entropy or args.tta is not None or smooth_of(args) is not None \
            or temperature_of(args) is not None:
        raise SystemExit("--propagate describes the labelled test pixels, not the scene: not with --out, --proba, --confidence, "
                         "--entropy, --tta, --smooth or --temperature")


def training_pixels(args, ck, job):
    """(spectra, labels) of the labelled training pixels on the device: the gallery of --knn_gallery train, --propagate's seeds"""
    if args.synthetic:          # the labelled split train.py --synthetic drew (its flags are in the checkpoint)
        from hsi_loader import SyntheticHSIDataSet
        saved = ck["extra"].get("args", {})
        scene = job.whole if (saved.get("windows") == "cube" or saved.get("synthetic_scene")) else None
        lab = SyntheticHSIDataSet(job.shape, saved.get("num_unlabel", 10000), 'label', seed=1, scene=scene)
    else:
        lab = HSIDataSet(int(args.dataID), 'label')
    return on_device(lab.X, torch.float32, job.device), on_device(lab.Y, torch.int64, job.device)


def labelled_spectra(job):
    """the spectra of the labelled test pixels, as the dataset keeps them"""
    rows = np.asarray(job.test_array, np.int64)
    return job.whole.X[rows] if torch.is_tensor(job.whole.X) else np.asarray(job.whole.X[rows])


def propagate_main(args, ck, job, hp, which, members, score=None):
    """--propagate: label propagation over the kNN graph of the embedding of the training and test pixels, per network of --net"""
    from cmlpl_amd.labelprop import propagate_embedding, score_labels
    K = job.shape[4]
    spectra, seeds = propagate_nodes(*training_pixels(args, ck, job), labelled_spectra(job), job.device)
    first, truth = len(seeds) - len(job.test_array), np.asarray(job.Y_test, np.int64)
    cfg = propagate_of(args)
    models = build_nets(job.shape, members, job.device, job.dropout)
    out = None
    for key, model in zip(which, models):
        model.eval()
        with torch.no_grad():
            graph, res = propagate_embedding(model, spectra, seeds, K, cfg, residual=True)[0]
        labels = res.labels[first:].cpu().numpy()
        tag = '_lp' + NET_TAGS[key]
        print('propagate%s: nodes=%d edges=%d max_in_degree=%d unreached=%d residual=%.3e' %
              (NET_TAGS[key], len(seeds), graph.edges(), graph.max_in_degree(), int((labels < 0).sum()), float(res.residual.cpu()[0])))
        print_block(tag, *score_labels(labels, truth, K)[:4])     # (an unreached node is -1: not CalAccuracy's to score)
        if score is not None:
            score(tag, res._replace(probs=res.probs[first:].clone()))      # (a buffer of its own: the test rows' block)
        out = labels if out is None else out
    return out


def knn_main(args, ck, job, hp, which, members, score=None):
    """--knn / --embed: the embedding of the labelled test pixels under the networks of --net, and its kNN vote"""
    from cmlpl_amd import NetShape
    from cmlpl_amd.knn import KnnEvaluator, embed
    Xt = on_device(labelled_spectra(job), torch.float32, job.device)
    Yt = on_device(np.asarray(job.Y_test), torch.int64, job.device)
    models = build_nets(job.shape, members, job.device, job.dropout)
    for model in models:
        model.eval()
    if args.embed:
        np.save(args.embed, embed(models[0], Xt)[0].cpu().numpy())
    if args.knn is None:
        return None
    loo = args.knn_gallery == 'loo'
    gallery = (Xt, Yt) if loo else training_pixels(args, ck, job)
    T = hp.get("temperature", 0.3) if args.knn_T is None else args.knn_T
    ev = KnnEvaluator(NetShape(*job.shape), *gallery, *((None, None) if loo else (Xt, Yt)), k=args.knn, T=T, loo=loo)
    first = None
    for key, model in zip(which, models):
        ev.evaluate(model)
        tag = '_knn' + NET_TAGS[key]
        labels = ev.last.labels[0].cpu().numpy()
        print_result(tag, labels, np.arange(len(job.test_array)), np.asarray(job.Y_test))
        if score is not None:
            score(tag, ev.last._replace(probs=ev.last.probs[0]))
        first = labels if first is None else first
    return first


def networks_of(args):
    """the networks --net names: keys of NET_TAGS, in the order of their blocks"""
    return {'both': [0, 1], 'ema_both': ['ema0', 'ema1'], **ENSEMBLES}.get(args.net) or \
        [args.net if args.net.startswith('ema') else int(args.net)]


# What a scene prediction does.  ``evaluate``: ``evaluate_whole`` first (networks one by one: their ``Result:`` blocks as ever).
# ``first_block`` None: nothing more; else one ``run_scene`` -- ``tta`` (None: ``ensemble_first``; of one network: its own softmax)
# under ``tag``, then ``stages`` = (('smooth' | 'superpixel' | 'region_graph' | 'temper' | 'sieve', its configuration), ..).  ``labels``: the map is the LAST
# stage's, the argmax of one network's logits from EVALUATE, or two such maps STACKED.
Plan = namedtuple('Plan', 'evaluate tta tag stages first_block labels')
LAST, EVALUATE, STACKED = 'last', 'evaluate', 'stacked'


def plan(args, has_test, noise=0.0):
    """the ``Plan`` of a checked command line; ``has_test``: the labelled test pixels exist; ``noise``: the default of --tta_noise"""
    temperature = temperature_of(args)
    if not has_test and (args.reliability or temperature == 'fit'):
        raise SystemExit("--reliability / --temperature fit need the labelled test pixels (test_array.npy and Y.npy in the "
                         "dataset directory)")
    tta = None if args.tta is None else TTA(args.tta, noise if args.tta_noise is None else args.tta_noise, seed=args.tta_seed,
                                            clean=not args.tta_no_clean, spatial=args.tta_spatial)
    together = tta is not None or args.net in ENSEMBLES
    tag = (NET_TAGS['ens'] if tta is None else tta_tag(tta)) if together else NET_TAGS[networks_of(args)[0]]
    # the regions vote behind --smooth and in front of --temperature, which tempers the FINAL probabilities; the sieve is last
    stages = tuple((name, cfg) for name, cfg in (('smooth', smooth_of(args)), ('superpixel', superpixel_of(args)),
                                                 ('region_graph', region_graph_of(args, len(networks_of(args)))),
                                                 ('temper', temperature), ('sieve', sieve_of(args))) if cfg is not None)
    if together:
        return Plan(False, tta, tag, stages, PRINT, LAST)
    # one network: its block comes from evaluate_whole; its own softmax is scored, handed to the stages or written, silently
    runs = stages or args.reliability or args.proba or args.confidence or args.entropy
    return Plan(True, None, tag, stages, (SCORE if args.reliability else SILENT) if runs else None,
                LAST if stages else STACKED if args.net in ('both', 'ema_both') else EVALUATE)


def build_stages(todo, job, args, fit=None):
    """the ``scene_report`` stages of ``Plan.stages``; ``fit``: the (rows, truth) on the device that --temperature fit fits on"""
    make = dict(smooth=smooth_stage, superpixel=lambda sp: superpixel_stage(sp, job, args.save_segments),
                region_graph=region_graph_stage, temper=lambda T: temper_stage(None if T == 'fit' else T, fit), sieve=sieve_stage)
    return [make[name](cfg) for name, cfg in todo]


def calibration(args, todo, job):
    """(fit, score) of a scene prediction: the (rows, truth) on the device that --temperature fit fits on -- a seeded share of
    the labelled test pixels -- and the ``RelScore`` of --reliability, which then counts on the held-out remainder (or None)"""
    fit = held = None
    if ('temper', 'fit') in todo.stages:
        fit, held = calibration_split(len(job.test_array), CALIB_FRAC if args.calib_frac is None else args.calib_frac,
                                      CALIB_SEED if args.calib_seed is None else args.calib_seed)
        if len(fit) < 1 or len(held) < 1:
            raise SystemExit("--temperature fit: the calibration share or its remainder is empty (%d labelled test pixels)" % len(job.test_array))
        fit = tuple(torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.int64)[fit])).to(job.device) for v in (job.test_array, job.Y_test))
    bins = REL_BINS if args.rel_bins is None else args.rel_bins
    return fit, RelScore(job.test_array, job.Y_test, job.device, bins, held) if args.reliability else None


def main(args, device=None):
    check_args(args)
    check_knn_args(args)
    check_propagate_args(args)
    if device is None:
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(device)
    ck = checkpoint.load(args.ckpt)
    s, hp = ck["identity"]["shape"], ck["identity"]["hp"]
    shape = (s["C"], s["H"], s["W"], s["bands"], s["K"])
    test_array = Y_test = None
    if args.synthetic:
        if tuple(SYNTH[args.synthetic]) != shape:
            raise SystemExit("--synthetic %s has shape %s, the checkpoint's networks take %s" %
                             (args.synthetic, SYNTH[args.synthetic], shape))
        whole = SyntheticScene(shape, 64, 64, seed=3)            # the scene train.py --synthetic evaluates on
        Y_test, test_array = whole.Y.numpy(), np.arange(len(whole))
    else:
        if DATASETS[int(args.dataID)] != (shape[4], shape[3]):
            raise SystemExit("--dataID %d has %d classes / %d bands, the checkpoint's networks take %d / %d" %
                             (args.dataID, *DATASETS[int(args.dataID)], shape[4], shape[3]))
        whole = HSIDataSet(int(args.dataID), 'wholeset')
        if os.path.exists(whole.root + 'test_array.npy') and os.path.exists(whole.root + 'Y.npy'):
            test_array = np.load(whole.root + 'test_array.npy')
            Y_test = (np.load(whole.root + 'Y.npy') - 1)[test_array]
    which = networks_of(args)
    todo = plan(args, test_array is not None, hp["noise"])
    if any(str(k).startswith('ema') for k in which) and ("Teacher" not in ck or "Teacher1" not in ck):
        raise SystemExit("--net %s: %s holds no EMA teacher (\"Teacher\" / \"Teacher1\"): it was written by a run "
                         "without train.py --ema" % (args.net, args.ckpt))
    keys = {0: "Base", 1: "Base1", 'ema0': "Teacher", 'ema1': "Teacher1"}
    job = SceneJob(shape, whole, device, args.synthetic, args.dataID, hp["dropout"], test_array, Y_test)
    members = [(k, ck[keys[k]]) for k in which]
    propagate = getattr(args, 'propagate', False)
    if args.knn is not None or args.embed or propagate:
        if test_array is None:
            raise SystemExit("--knn / --embed / --propagate need the labelled test pixels (test_array.npy and Y.npy in the dataset "
                             "directory)")
        # (the blocks are over the test LIST: position i of a probability map is test pixel i)
        score = RelScore(np.arange(len(test_array)), Y_test, device, REL_BINS if args.rel_bins is None else args.rel_bins) \
            if args.reliability else None
        out = None
        for stage in [knn_main] * (args.knn is not None or bool(args.embed)) + [propagate_main] * bool(propagate):  # _knn, then _lp
            labels = stage(args, ck, job, hp, which, members, score=score)
            out = labels if out is None else out
        if args.save_reliability and (args.knn is not None or propagate):
            score.save(args.save_reliability)
        return out
    fit, score = calibration(args, todo, job)
    preds = evaluate_whole(job, members, val_batch_size=args.val_batch_size) if todo.evaluate else None
    out = {}
    if todo.first_block is not None:
        if todo.first_block == SILENT and not todo.stages:     # (nothing is printed: the softmax is only written)
            job = job._replace(test_array=None)
        first = ensemble_first(todo.tag) if todo.tta is None else tta_first(todo.tta)
        out = run_scene(job, members, first, build_stages(todo.stages, job, args, fit), first_block=todo.first_block, score=score,
                        want=dict(probs=bool(args.proba), conf=bool(args.confidence), entropy=bool(args.entropy)))
    if todo.labels != LAST:         # (a network nothing re-labels keeps the argmax of its logits as its label map)
        labels = np.stack([preds[k] for k in which]).astype(np.int64)
        out["labels"] = labels if todo.labels == STACKED else labels[0]
    for path, key in ((args.proba, "probs"), (args.confidence, "conf"), (args.entropy, "entropy")):
        if path:
            np.save(path, out[key])
    if args.out:
        np.save(args.out, out["labels"])
    if args.save_reliability:
        score.save(args.save_reliability)
    return out["labels"]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument('--ckpt', required=True, help='a checkpoint of train.py --save_ckpt / --save_best')
    parser.add_argument('--dataID', type=int, default=1)
    parser.add_argument('--net', choices=('0', '1', 'both', 'ema0', 'ema1', 'ema_both', 'ensemble', 'ensemble_all'),
                        default='0',
                        help="Base (0), Base1 (1) or both; ema0 / ema1 / ema_both: their EMA teachers (a checkpoint of "
                             "train.py --ema); ensemble: Base and Base1 together, one label map from their averaged "
                             "softmax; ensemble_all: with both EMA teachers")
    parser.add_argument('--out', default=None, help='write the int64 label map as .npy ([rows*cols]; both: [2][rows*cols])')
    parser.add_argument('--proba', default=None, metavar='FILE',
                        help='write the class probabilities float32 [rows*cols, K] as .npy (the ensemble\'s, or one '
                             'network\'s own softmax; not with both / ema_both)')
    parser.add_argument('--confidence', default=None, metavar='FILE',
                        help='write the probability of the predicted class float32 [rows*cols] as .npy')
    parser.add_argument('--entropy', default=None, metavar='FILE',
                        help='write the entropy of the class probabilities float32 [rows*cols] as .npy')
    parser.add_argument('--tta', type=int, default=None, metavar='M',
                        help='test-time augmentation: predict from the clean window and M noisy views of every pixel, '
                             'averaged over the views and the networks of --net (not with both / ema_both)')
    parser.add_argument('--tta_noise', type=float, default=None, metavar='S',
                        help="--tta: the views are x + S N(0,1) (default: the checkpoint's training noise)")
    parser.add_argument('--tta_seed', type=int, default=1088, metavar='N', help='--tta: the seed of the views')
    parser.add_argument('--tta_no_clean', action='store_true', help='--tta: the noisy views only, without the clean window')
    parser.add_argument('--tta_spatial', choices=SPATIAL_MODES, default='none',
                        help="--tta: the views are also flipped ('flips': 4 elements) or flipped and rotated ('d4': 8) windows, "
                             "view t under element (t + 1) mod 4 / 8 (t mod 4 / 8 with --tta_no_clean); with --tta_noise 0 pure "
                             "geometry; the Result: tag becomes _tta_flips / _tta_d4")
    add_smooth_flags(parser, 'the prediction of --net (with or without --tta; not with both / ema_both)')
    add_superpixel_flags(parser, 'the prediction of --net (with or without --tta, behind --smooth; not with both / ema_both)')
    add_region_graph_flags(parser, 'the prediction of --net (not with both / ema_both)')
    add_sieve_flags(parser, 'the prediction of --net (with or without --tta; not with both / ema_both, not with --entropy)')
    parser.add_argument('--reliability', action='store_true',
                        help='behind every Result: block one line Reliability<tag>: ECE, MCE, NLL, Brier score, mean confidence '
                             'and accuracy of the block\'s class probabilities over the labelled test pixels (not with both / '
                             'ema_both)')
    parser.add_argument('--rel_bins', type=int, default=None, metavar='B',
                        help='--reliability: the number of confidence bins (default 15, 1 .. 1024)')
    parser.add_argument('--save_reliability', default=None, metavar='FILE',
                        help='--reliability: write the int64 counter blocks as .npz, one entry Reliability<tag> per line '
                             '(cmlpl_amd.calibrate.Reliability names the fields)')
    parser.add_argument('--temperature', default=None, metavar='T',
                        help="temper the final class probabilities of the prediction, q = softmax(log p / T): one more Result: "
                             "block, tag ..._T; 'fit': the T of the least NLL on a share of the labelled test pixels")
    parser.add_argument('--calib_frac', type=float, default=None, metavar='F',
                        help='--temperature fit: the share of the labelled test pixels that fits T (default 0.5); every '
                             'Reliability line is then counted on the remainder')
    parser.add_argument('--calib_seed', type=int, default=None, metavar='N',
                        help='--temperature fit: the seed of that share (default 1088)')
    parser.add_argument('--knn', type=int, default=None, metavar='K',
                        help='score the embedding: the weighted kNN vote (K neighbours) of the labelled test pixels, one Result: '
                             'block per network of --net with the tag _knn (not with the ensembles)')
    parser.add_argument('--knn_T', type=float, default=None, metavar='T',
                        help="--knn: the temperature of the vote (default: the checkpoint's training temperature)")
    parser.add_argument('--knn_gallery', choices=('train', 'loo'), default=None,
                        help="--knn: the gallery -- the labelled training pixels (train, the default) or leave-one-out among the "
                             "test pixels (loo)")
    parser.add_argument('--embed', default=None, metavar='FILE',
                        help='write the float32 [n_test][1024] embedding of the labelled test pixels under a single network as .npy')
    add_propagate_flags(parser, 'one propagate line and one Result: block per network of --net with the tag _lp (not with the '
                                'ensembles)')
    parser.add_argument('--val_batch_size', type=int, default=512,
                        help='batch of the loader fall-back (a dataset directory without cube.npy)')
    parser.add_argument('--synthetic', choices=sorted(SYNTH), default=None,
                        help="label the seeded synthetic scene of this shape (train.py --synthetic's evaluation scene)")
    return parser


if __name__ == '__main__':
    main(build_parser().parse_args())
