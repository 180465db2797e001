#!/usr/bin/env python3
"""CMLPL training driver on MI355X -- same command line as the reference's ``train.py``
(flags of train.py:356-379, printed line of train.py:282-289), with the per-step hot path
(train.py:150-278) executed by ``cmlpl_amd.TrainEngine`` (hand-written gfx950 kernels).

Differences from the reference that are deliberate, MI355X-first choices:
  * the labelled / unlabelled splits live in HBM for the whole run and a batch is a list of row INDICES into them
    (the epoch's permutation, also resident): the kernels read the rows where they lie, no batch tensor is gathered
    (the reference copies every batch over PCIe and draws noise on the CPU);
  * ``--graph``: the step is captured once as a hipGraph and replayed, one launch per step, its per-step scalars
    coming from a device-side table filled once per epoch (several GPUs: one graph per stage of the sharded step,
    the collectives eager between them -- cmlpl_amd.distributed.DistStepGraph);
  * noise and dropout come from in-kernel counter-based streams (PCG4D hash + Box-Muller for the augmentation noise,
    Philox4x32-10 for the dropout masks) seeded with the reference's seed 1088;
  * the five logged scalars of every step (loss_hist, train.py:136,274-278) are written by the step into a
    device-side ring and read back once per ``print_per_batches`` steps, not five times a step; the printed line
    is the mean over that window, as in train.py:281-289.
  * ``--windows cube``: no window tensor at all -- the scene cube (cube.npy, 50 MB for PaviaU) is uploaded once and every
    step, eager or replayed, on one or several GPUs, gathers its windows from it (the cube-fed step of cmlpl_amd); the
    default ``--windows split`` cuts each split's windows once and keeps them resident (2 x 960 MB at the defaults).
  * ``--eval_every N``: after every N-th epoch both networks are scored on the TEST split's pixels, on the device
    (cmlpl_amd.evaluate.Evaluator: the list-fed eval forward from the scene cube, both networks in one call, the confusion
    matrices counted there); one line per network with OA / AA / Kappa, the curve to ``--save_eval``.  Default 0: never.
  * ``--method cps``: the cross-pseudo-supervision baseline of the reference's ``trian_CPS.py`` instead of CMLPL, on the
    same two networks, loaders, evaluation and checkpoints (one GPU; ``trian_CPS.py`` here presets it).  The printed
    line is the shared one: for CPS ``loss_contrast`` repeats ``con_loss`` (trian_CPS.py:254).
  * ``--ema``: an exponential moving average of both networks' weights (the reference's ``WeightEMA_BN``, coefficient
    ``--teacher_alpha``) is kept on the device, updated behind every step (one launch; also behind a graph replay), scored
    by ``--eval_every`` on two more lines (``validation_ema`` / ``validation_ema1``), saved with every checkpoint
    (``"Teacher"`` / ``"Teacher1"``) and evaluated after the run.  One GPU.  Without it ``--teacher_alpha`` is ignored.
  * ``--ensemble``: the two networks are also scored TOGETHER -- the label of their averaged softmax
    (cmlpl_amd.ensemble, one launch behind the eval forward): a third ``validation_ens`` line per ``--eval_every``
    evaluation, a curve of its own in ``--save_eval`` and the checkpoints, a third ``Result:`` block (``OA_ens``) after
    the run.  It reads the networks and changes nothing they compute: ``loss_hist`` is what it is without the flag.
  * ``--smooth R``: after the run Base and Base1 are scored together once more with their class probability maps
    SMOOTHED over the scene -- an edge-preserving filter of radius R guided by the cube's leading principal components
    (cmlpl_amd.smooth; ``--smooth_sigma_s`` / ``--smooth_sigma_r`` / ``--smooth_guide`` / ``--smooth_iters``): one more
    ``Result:`` block (``OA_ens_smooth``).  The run itself is untouched.
  * ``--superpixel S``: after the run Base and Base1 are scored together once more as REGIONS -- the scene is over-segmented
    into superpixels on a grid of step S under the cube's leading principal components and every region votes as one
    (cmlpl_amd.superpixel; ``--sp_compact`` / ``--sp_iters`` / ``--sp_guide`` / ``--sp_vote`` / ``--save_segments``): a
    ``superpixel:`` line (segments, empty ones, sizes, ASA) and one more ``Result:`` block (``OA_ens_sp``; behind ``--smooth``:
    ``OA_ens_smooth_sp``).  One GPU.  The run itself is untouched and no checkpoint records the flag.  ``--sp_connect``: the
    regions that vote are CONNECTED -- detached fragments of fewer than S S / 4 pixels join the largest region they touch and
    every remaining component is a segment of its own (cmlpl_amd.regions.connect_segments); the ``superpixel:`` line then
    describes that map and a line ``superpixel connectivity: components_before= fragments_merged= segments=`` follows it.
  * ``--region_graph`` (``--rg_k K``, ``--rg_adj A``, ``--rg_alpha a``, ``--rg_gamma g``, ``--rg_iters T``, ``--rg_net i``), with
    ``--superpixel S``: the regions that voted become the nodes of a label propagation -- every region is described by the
    embedding of its mean spectrum under member i, linked to its K most similar and its A adjacent regions (by shared
    boundary length), and the vote is the prior that diffuses (cmlpl_amd.regiongraph).  One ``region graph:`` line (nodes, knn,
    adj, edges, max_in_degree, truncated, unreached, residual) and one more ``Result:`` block (``OA_ens_sp_rg``; behind
    ``--smooth``: ``OA_ens_smooth_sp_rg``).  One GPU.  The run itself is untouched and no checkpoint records the flag.  The
    defaults are not tuned.
  * ``--sieve N`` (``--sieve_conn 4 | 8``, ``--sieve_passes T``): after the run the label map of Base and Base1 together --
    behind ``--smooth`` and ``--superpixel`` when given -- is SIEVED: a connected region of fewer than N pixels takes the label
    of the largest region of at least N pixels that it touches (cmlpl_amd.regions; the operation GDAL calls sieve).  One
    ``sieve:`` line (components, small ones, pixels relabelled, passes used, components left) and one more ``Result:`` block
    (``OA_ens_sv``, ``OA_ens_smooth_sv``, ..).  One GPU.  The run itself is untouched and no checkpoint records the flag.  An N
    near the size of the true regions removes them; what the sieve buys on a real scene is not measured.
  * ``--aug_spatial flips | d4``: flip (and rotate) augmentation of the training windows, the reference's ``flip`` /
    ``Random_rot`` (hsi_loader.py:58-88): every batch row takes one element of the dihedral group per step, the same for
    both networks, applied inside the gather of ``--windows cube`` (which it needs; one GPU).  ``--tta --tta_spatial
    flips | d4`` scores such views after the run (``OA_tta_flips`` / ``OA_tta_d4``).
  * ``--pl_stats``: the pseudo-label monitor -- every step's targets are scored against the TRUTH of its unlabelled rows (the
    loader carries the unlabelled split's labels; the reference never reads them), on the device, one launch behind every
    step, eager or replayed (``TrainEngine(pl_monitor=True)``).  After every epoch one ``pl_stats`` line: per direction
    (Base's targets, then Base1's, suffix ``1``) the rows the mask selected, the accuracy of the selected pseudo-labels, of
    all of them and of the plain softmax's (what memory-bank smoothing changed); for CMLPL also the positive and negative
    edges of the pseudo-label graph and their precision.  ``--save_pl PATH``: the per-epoch counter blocks.  One GPU.  The
    run itself is untouched: ``loss_hist`` is what it is without the flag.
  * ``--reliability``: behind every ``_ens`` / ``_tta..`` / ``.._smooth`` block of the end-of-run report one ``Reliability<tag>:``
    line -- ECE, MCE, NLL, Brier score, mean confidence and accuracy of that block's class probabilities over the labelled
    test pixels, from integer counters kept on the device (cmlpl_amd.calibrate).  It needs ``--ensemble``, ``--tta`` or
    ``--smooth`` (or ``--superpixel``, whose ``.._sp`` block it scores as well); ``loss_hist``, checkpoints and every other line
    are what they are without the flag.
  * ``--knn K`` (``--knn_T T``, default ``--temperature``): the embedding itself is scored -- the weighted kNN vote
    (cmlpl_amd.knn: K neighbours by cosine similarity of the spectral branch's ``feat``, each weighted by exp(s / T)) of the
    test split's pixels over the labelled training pixels, untiled.  With ``--eval_every`` two more lines per evaluation
    (``validation_knn`` / ``validation_knn1``) and a curve of its own (``curve_knn`` in ``--save_eval``; in the checkpoints,
    restored by ``--resume``); the same two lines once after the last epoch.  One GPU; ``loss_hist`` is what it is without it.
  * ``--propagate`` (``--lp_k K``, ``--lp_alpha A``, ``--lp_gamma G``, ``--lp_iters N``; defaults 10, 0.99, 3, 50, not tuned): a
    second opinion on the classifier that costs no training -- label propagation over the embedding's kNN graph
    (cmlpl_amd.labelprop: the labelled training pixels are the seeds, the test split's pixels the other nodes), once after
    the last epoch: two lines ``validation_lp`` / ``validation_lp1`` in the format of ``validation_knn``.  One GPU; ``loss_hist``,
    the curves, the checkpoints (the flag is not recorded in them) and every other line are what they are without it.
  * ``--lr_schedule constant | linear | cosine`` (``--warmup_steps N``, ``--lr_min F``), ``--weight_decay F``, ``--clip_grad F``:
    a learning-rate schedule over the run's steps (linear warm-up, then the decay; cmlpl_amd.optim.LRSchedule), AdamW's
    decoupled weight decay, and gradient-norm clipping per network (torch's ``clip_grad_norm_``; one launch more per step,
    eager or replayed).  With any of them on, one ``optim`` line per epoch -- the last rate, mean and max of each network's
    gradient norm, how many steps clipped -- and ``--save_optim PATH`` writes [num_steps][5] = lr, norm, norm1, coef, coef1.
    One GPU.  The defaults are the reference's fixed-rate Adam: no line, no launch, and a checkpoint is what it was.
``--synthetic SHAPE`` (B2 | P | B4 | B5) runs without the datasets, which are not shipped.
Multi-GPU: ``python -m torch.distributed.run --nproc-per-node N train.py ...`` shards every batch by
sample over the ranks (cmlpl_amd.distributed); batch sizes must be multiples of N, and a short last batch
is cut to the largest equal shards (see shard_plan)."""
import argparse
import os
import time

import numpy as np
import torch

from cmlpl_amd import HyperParams, NetShape, checkpoint
from hsi_loader import HSIDataSet, SyntheticHSIDataSet, SyntheticScene
from scene_report import (NET_TAGS, PRINT, SILENT, SMOOTH_TAG, SP_TAG, RelScore, SceneJob, build_nets, calibration_split,  # noqa: F401
                          ensemble_first, evaluate_whole, region_graph_stage, run_scene, sieve_stage, smooth_stage, superpixel_stage, tta_first, tta_tag, tta_timing)

DATASETS = {1: (9, 103), 2: (16, 204), 3: (15, 144), 4: (16, 200)}     # num_classes, num_features (train.py:75-90)
SYNTH = {"B2": (103, 11, 11, 103, 9), "P": (60, 20, 20, 103, 9), "B4": (200, 11, 11, 200, 16),
         "B5": (48, 15, 15, 48, 20), "W8": (40, 8, 8, 40, 5)}


class DeviceLoader:
    """shuffle=True DataLoader semantics (one random permutation per epoch, last short batch kept)
    over arrays that already sit in HBM.  A batch is (offset, size) into ``self.perm``, the epoch's permutation in a
    FIXED device buffer (a captured step keeps reading the same buffer): the step takes the rows by index."""

    def __init__(self, arrays, batch_size, generator):
        self.XP, self.X, self.Y = arrays
        self.bs, self.g = batch_size, generator
        self.perm = torch.zeros(len(self.X), dtype=torch.int64, device=self.X.device)

    def __len__(self):
        return (len(self.X) + self.bs - 1) // self.bs

    def __iter__(self):
        # (stream-ordered behind the previous epoch's steps, which still read the buffer)
        self.perm.copy_(torch.randperm(len(self.X), generator=self.g))
        for i in range(0, len(self.X), self.bs):
            yield i, min(self.bs, len(self.X) - i)

    def rows(self, off, size):
        """the gathered batch (engines that do not take indices: the CPU stand-in of the tests)"""
        idx = self.perm[off:off + size]
        return self.XP[idx], self.X[idx], self.Y[idx]


def shard_plan(bt, btu, world):
    """How a GLOBAL batch of bt + btu rows is taken by `world` ranks: (bt_l, btu_l) rows per rank, or None when the
    batch cannot be sharded equally.  Decided from the global sizes only, so every rank decides the same way (a rank
    that skipped a step others ran would leave them waiting in a collective).  Equal shards are required because
    the ranks' loss shares are summed into global means; the rows that do not divide are dropped,
    the pointer/step bookkeeping still advances on every rank alike."""
    bt_l, btu_l = bt // world, btu // world
    if bt_l < 1 or btu_l < 1:
        return None
    return bt_l, btu_l


RUN_FLAGS = ("lr", "num_epochs", "thr", "alpha", "queue_batch", "temperature", "dropout", "noise",
             "labeled_batch_size", "unlabeled_batch_size", "num_unlabel")


def run_record(args, hp, shape, from_scene):
    """what two legs of one run (--resume) must agree on: the hyper-parameter flags (--num_epochs too: the threshold
    schedule adap_thr(epoch) divides by it), the batch sizes and the data.  --graph, --windows, --eval_every,
    --print_per_batches and the number of GPUs may differ."""
    rec = {k: getattr(args, k) for k in RUN_FLAGS}
    if args.method != "cmlpl":            # (a CMLPL run's record is what it was before there was a second method)
        rec["method"] = args.method
    if args.ema:                          # (and a run without a teacher's is what it was before there was one)
        rec.update(ema=True, teacher_alpha=args.teacher_alpha)
    if args.aug_spatial != "none":        # (and a run on windows as they are)
        rec["aug_spatial"] = args.aug_spatial
    rec.update(shape=[int(v) for v in shape], data=("synthetic %s%s" % (args.synthetic, " scene" if from_scene else ""))
               if args.synthetic else "dataID %d" % int(args.dataID))
    return rec


def saved_args(args):
    """the command line as a checkpoint keeps it: a flag that came after the format (--method, --ema, --ensemble, --tta, --smooth and
    its sub-flags, --aug_spatial, --tta_spatial, --pl_stats, --save_pl, --reliability, --knn, --knn_T, the optimiser flags) is left out at its default, so a file written without it is byte for byte what it
    was before the flag existed; --propagate, --superpixel, --region_graph, --sieve and their sub-flags only add lines behind the run and are never recorded"""
    late = {'method': 'cmlpl', 'ema': False, 'ensemble': False, 'tta': False, **{k: None for k in SMOOTH_FLAGS},
            'aug_spatial': 'none', 'tta_spatial': 'none', 'pl_stats': False, 'save_pl': None, 'reliability': False,
            'knn': None, 'knn_T': None, **OPTIM_FLAGS}
    return {k: v for k, v in vars(args).items() if not (k in late and v == late[k]) and k not in LP_FLAGS and k not in SP_FLAGS
            and k not in SIEVE_FLAGS and k not in RG_FLAGS}


LP_FLAGS = ('propagate', 'lp_k', 'lp_alpha', 'lp_gamma', 'lp_iters')     # --propagate: cmlpl_amd.labelprop.LabelProp's fields


def add_propagate_flags(parser, what):
    """``--propagate`` and its sub-flags (train.py and predict.py); every sub-flag's default is None: the flag was not given"""
    parser.add_argument('--propagate', action='store_true',
                        help='label propagation over the kNN graph of the spectral embedding (cmlpl_amd.labelprop): the labelled '
                             'training pixels are the seeds, the labelled test pixels the other nodes; %s (one GPU)' % what)
    parser.add_argument('--lp_k', type=int, default=None, metavar='K', help='--propagate: neighbours per node (default 10, 1 .. 32)')
    parser.add_argument('--lp_alpha', type=float, default=None, metavar='A',
                        help='--propagate: the share a node takes from its neighbours per iteration (default 0.99, 0 <= A < 1)')
    parser.add_argument('--lp_gamma', type=int, default=None, metavar='G',
                        help='--propagate: an edge weighs similarity^G (default 3, 1 .. 8)')
    parser.add_argument('--lp_iters', type=int, default=None, metavar='N', help='--propagate: iterations (default 50, 1 .. 10000)')


def propagate_of(args):
    """the ``cmlpl_amd.labelprop.LabelProp`` of the command line, or None without ``--propagate``; what it cannot mean is a
    SystemExit before anything is loaded"""
    given = [k for k in LP_FLAGS[1:] if getattr(args, k, None) is not None]
    if not getattr(args, 'propagate', False):
        if given:
            raise SystemExit("%s belong%s to --propagate" % (" / ".join("--" + k for k in given), "s" if len(given) == 1 else ""))
        return None
    from cmlpl_amd.labelprop import LabelProp
    cfg = LabelProp(**{k[3:]: getattr(args, k) for k in given})
    try:
        return cfg.check()
    except ValueError as e:
        raise SystemExit("--propagate: --lp_%s" % e)


def on_device(a, dt, device):
    """a tensor or array as a contiguous tensor of dtype ``dt`` on ``device``"""
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dt).to(device).contiguous()


def propagate_nodes(seeds_X, seeds_Y, test_X, device):
    """the nodes of --propagate: (spectra float32 [n, bands], seed labels int64 [n], -1 for a test pixel) -- the labelled
    training pixels followed by the labelled test pixels"""
    seeds_X, seeds_Y, test_X = (on_device(a, dt, device) for a, dt in
                                ((seeds_X, torch.float32), (seeds_Y, torch.int64), (test_X, torch.float32)))
    return (torch.cat([seeds_X, test_X]).contiguous(),
            torch.cat([seeds_Y, torch.full((test_X.shape[0],), -1, dtype=torch.int64, device=device)]))


OPTIM_FLAGS = {'lr_schedule': 'constant', 'warmup_steps': 0, 'lr_min': 0.0, 'weight_decay': 0.0, 'clip_grad': 0.0,
               'save_optim': None}     # the flags of cmlpl_amd.optim, at their defaults: the reference's fixed-rate Adam


def optim_of(args, total_steps):
    """the run's ``cmlpl_amd.optim.OptimConfig``, or None with every optimiser flag at its default; ``total_steps``: the
    steps of the WHOLE run (--num_epochs epochs), which a resumed leg shares with the leg that wrote its file"""
    from cmlpl_amd.optim import LRSchedule, OptimConfig
    try:
        schedule = None
        if args.lr_schedule != 'constant' or args.warmup_steps != 0:
            schedule = LRSchedule(args.lr_schedule, args.lr, total_steps, warmup_steps=args.warmup_steps, lr_min=args.lr_min)
        elif args.lr_min != 0.0:
            raise ValueError("--lr_min belongs to --lr_schedule linear | cosine")
        cfg = OptimConfig(schedule=schedule, weight_decay=args.weight_decay, clip_grad=args.clip_grad)
    except ValueError as e:
        raise SystemExit("optimiser flags: %s" % e)
    return cfg if cfg.active() else None


def optim_line(epoch, num_epochs, rows):
    """the ``optim`` line of one epoch's rows [steps][5] = lr, norm, norm1, coef, coef1"""
    parts = ['lr = %.4e' % rows[-1, 0]]
    for d, tag in enumerate(('', '1')):
        parts.append('norm%s = %.4f max%s = %.4f clipped%s = %d/%d' %
                     (tag, rows[:, 1 + d].mean(), tag, rows[:, 1 + d].max(), tag, int((rows[:, 3 + d] < 1.0).sum()), len(rows)))
    return 'Epoch %d/%d: optim %s' % (epoch, num_epochs, ' '.join(parts))


def run_differences(saved, mine):
    keys = list(mine) + [k for k in ("ema", "teacher_alpha", "aug_spatial") if k in saved and k not in mine]     # --ema, --aug_spatial: both ways
    return ["%s: file %r, here %r" % (k, saved.get(k), mine.get(k)) for k in keys if saved.get(k) != mine.get(k)]


class EvalCurve:
    """One validation curve of --eval_every: the epochs that were scored, a row per evaluation and its confusion matrices.
    ``nets`` = 2: a row is [net][OA, AA, Kappa] and the matrices are [2, K, K] (the two networks, suffix ''; their EMA
    teachers, '_ema'); ``nets`` = None: a row is [OA, AA, Kappa] and the matrix [K, K] (the pair together, '_ens').  The
    suffix names the curve in a checkpoint's ``extra``, in --save_eval and on the printed lines."""

    def __init__(self, suffix, nets):
        self.suffix, self.nets, self.epochs, self.rows, self.cms = suffix, nets, [], [], []

    def add(self, epoch, row, cm):
        self.epochs.append(epoch)
        self.rows.append(row)
        self.cms.append(cm)

    def restore(self, extra):
        """the curve so far, from a checkpoint's ``extra``; a file without this curve leaves it empty"""
        if "eval_curve" + self.suffix in extra:
            self.epochs = [int(e) for e in extra["eval_epochs" + self.suffix]]
            self.rows = extra["eval_curve" + self.suffix].tolist()
            self.cms = list(extra["eval_cms" + self.suffix].numpy())

    def checkpoint_entries(self, num_classes):
        """eval_epochs / eval_curve (float64 [E, nets, 3]) / eval_cms (int64 [E, nets, K, K]); no ``nets`` axis for the pair"""
        per = () if self.nets is None else (self.nets,)
        return {"eval_epochs" + self.suffix: list(self.epochs),
                "eval_curve" + self.suffix: torch.tensor(self.rows, dtype=torch.float64).reshape(len(self.epochs), *per, 3),
                "eval_cms" + self.suffix: torch.from_numpy(np.stack(self.cms)) if self.cms else
                torch.zeros(0, *per, num_classes, num_classes, dtype=torch.int64)}

    def npz_entries(self):
        """the members of --save_eval, in the order the file has had them (the first curve's differs from the later two's)"""
        members = dict(curve=np.array(self.rows), cm=np.stack(self.cms), epochs=np.array(self.epochs))
        return {k + self.suffix: members[k] for k in (("curve", "cm", "epochs") if self.suffix else ("curve", "epochs", "cm"))}

    def best_line(self, net=None):
        """the ``best validation`` line of network ``net``: the epoch and the OA of its best-scored evaluation (the first of equal bests)"""
        oa = np.array(self.rows)[..., 0] if net is None else np.array(self.rows)[:, net, 0]
        return 'best validation%s%s: epoch %d OA = %.2f' % (self.suffix, NET_TAGS[net or 0], self.epochs[int(np.argmax(oa))], oa.max() * 100)


SPATIAL_MODES = ('none', 'flips', 'd4')                            # --aug_spatial / --tta_spatial (cmlpl_amd._lib.SPATIAL)
SMOOTH_FLAGS = ('smooth', 'smooth_sigma_s', 'smooth_sigma_r', 'smooth_guide', 'smooth_iters')


def add_smooth_flags(parser, what):
    """``--smooth R`` and its sub-flags (train.py and predict.py); every default is None: the flag was not given"""
    parser.add_argument('--smooth', type=int, default=None, metavar='R',
                        help='edge-preserving spatial smoothing of the class probability maps of %s, radius R (1 .. 8), guided '
                             'by the leading channels of the scene cube: one more Result: block, tag ..._smooth' % what)
    parser.add_argument('--smooth_sigma_s', type=float, default=None, metavar='S',
                        help='--smooth: the spatial width in pixels (default R / 2)')
    parser.add_argument('--smooth_sigma_r', type=float, default=None, metavar='S',
                        help="--smooth: the width in the guide's z-scored units (default 0.5; inf: the guide does not count)")
    parser.add_argument('--smooth_guide', type=int, default=None, metavar='G',
                        help='--smooth: how many leading channels of the cube guide the filter (default 3, 0 .. 8; 0: none)')
    parser.add_argument('--smooth_iters', type=int, default=None, metavar='N', help='--smooth: passes of the filter (default 1)')


def smooth_of(args):
    """the ``cmlpl_amd.smooth.Smooth`` of the command line, or None without ``--smooth``; what it cannot mean is a SystemExit
    before anything is loaded"""
    given = [k for k in SMOOTH_FLAGS[1:] if getattr(args, k, None) is not None]
    if getattr(args, 'smooth', None) is None:
        if given:
            raise SystemExit("%s belong%s to --smooth R" % (" / ".join("--" + k for k in given), "s" if len(given) == 1 else ""))
        return None
    from cmlpl_amd.smooth import Smooth
    asked = {k: getattr(args, 'smooth_' + k, None) for k in ('sigma_s', 'sigma_r', 'guide', 'iters')}
    smooth = Smooth(args.smooth, **{k: v for k, v in asked.items() if v is not None})
    try:
        smooth.params()
    except ValueError as e:
        raise SystemExit("--smooth: %s" % str(e).replace("Smooth: ", ""))
    return smooth


SP_FLAGS = ('superpixel', 'sp_compact', 'sp_iters', 'sp_guide', 'sp_vote', 'save_segments', 'sp_connect')
SIEVE_FLAGS = ('sieve', 'sieve_conn', 'sieve_passes')


def add_superpixel_flags(parser, what):
    """``--superpixel S`` and its sub-flags (train.py and predict.py); every default is None: the flag was not given"""
    parser.add_argument('--superpixel', type=int, default=None, metavar='S',
                        help='object-based classification of %s: the scene is over-segmented into superpixels on a grid of '
                             'step S (2 .. 64) under the leading channels of the scene cube, and every region votes as one: '
                             'one more Result: block, tag ..._sp' % what)
    parser.add_argument('--sp_compact', type=float, default=None, metavar='M',
                        help='--superpixel: the compactness, the weight of the distance in the image (default 1)')
    parser.add_argument('--sp_iters', type=int, default=None, metavar='T',
                        help='--superpixel: rounds of assign and update (default 10, 1 .. 100)')
    parser.add_argument('--sp_guide', type=int, default=None, metavar='G',
                        help='--superpixel: how many leading channels of the cube guide the segmentation (default 3, 0 .. 8; 0: '
                             'a plain grid)')
    parser.add_argument('--sp_vote', choices=('soft', 'hard'), default=None,
                        help="--superpixel: a region sums its pixels' class probabilities (soft, the default) or counts their "
                             "labels (hard)")
    parser.add_argument('--save_segments', default=None, metavar='FILE',
                        help='--superpixel: write the int32 segment map [rows*cols] as .npy')
    parser.add_argument('--sp_connect', action='store_const', const=True, default=None,
                        help='--superpixel: the regions that vote are connected -- fragments of fewer than S S / 4 pixels join the '
                             'largest region they touch, every remaining component is a segment of its own')


def superpixel_of(args):
    """the ``cmlpl_amd.superpixel.Superpixel`` of the command line, or None without ``--superpixel``; what it cannot mean is
    a SystemExit before anything is loaded"""
    given = [k for k in SP_FLAGS[1:] if getattr(args, k, None) is not None]
    if getattr(args, 'superpixel', None) is None:
        if given:
            raise SystemExit("%s belong%s to --superpixel S" % (" / ".join("--" + k for k in given), "s" if len(given) == 1 else ""))
        return None
    from cmlpl_amd.superpixel import Superpixel
    asked = {k: getattr(args, 'sp_' + k, None) for k in ('compact', 'iters', 'guide', 'vote', 'connect')}
    sp = Superpixel(args.superpixel, **{k: v for k, v in asked.items() if v is not None})
    try:
        sp.params()
    except ValueError as e:
        raise SystemExit("--superpixel: %s" % str(e).replace("Superpixel: ", ""))
    return sp


def add_sieve_flags(parser, what):
    """``--sieve N`` and its sub-flags (train.py and predict.py); every default is None: the flag was not given"""
    parser.add_argument('--sieve', type=int, default=None, metavar='N',
                        help='sieve the label map of %s, behind every other stage: a connected region of fewer than N pixels '
                             'takes the label of the largest region of at least N pixels that it touches: one sieve: line and '
                             'one more Result: block, tag ..._sv' % what)
    parser.add_argument('--sieve_conn', type=int, choices=(4, 8), default=None, help='--sieve: 4- (the default) or 8-connected regions')
    parser.add_argument('--sieve_passes', type=int, default=None, metavar='T',
                        help='--sieve: passes (default 4, 1 .. 16); a pass that moves nothing ends the effect')


def sieve_of(args):
    """the ``cmlpl_amd.regions.Sieve`` of the command line, or None without ``--sieve``; what it cannot mean is a SystemExit
    before anything is loaded"""
    given = [k for k in SIEVE_FLAGS[1:] if getattr(args, k, None) is not None]
    if getattr(args, 'sieve', None) is None:
        if given:
            raise SystemExit("%s belong%s to --sieve N" % (" / ".join("--" + k for k in given), "s" if len(given) == 1 else ""))
        return None
    from cmlpl_amd.regions import Sieve
    asked = dict(conn=getattr(args, 'sieve_conn', None), passes=getattr(args, 'sieve_passes', None))
    sv = Sieve(args.sieve, **{k: v for k, v in asked.items() if v is not None})
    try:
        sv.params()
    except ValueError as e:
        raise SystemExit("--sieve: %s" % str(e).replace("Sieve: ", ""))
    return sv


RG_FLAGS = ('region_graph', 'rg_k', 'rg_adj', 'rg_alpha', 'rg_gamma', 'rg_iters', 'rg_net')    # cmlpl_amd.regiongraph.RegionGraph's fields


def add_region_graph_flags(parser, what):
    """``--region_graph`` and its sub-flags (train.py and predict.py); every sub-flag's default is None: the flag was not given"""
    parser.add_argument('--region_graph', action='store_const', const=True, default=None,
                        help='--superpixel: the regions that voted become the nodes of a label propagation over their most '
                             'similar (embedding of the mean spectrum) and their adjacent regions, the vote is its prior: one '
                             'region graph: line and one more Result: block, tag ..._rg, for %s' % what)
    parser.add_argument('--rg_k', type=int, default=None, metavar='K', help='--region_graph: kNN neighbours per region (default 8, 0 .. 32)')
    parser.add_argument('--rg_adj', type=int, default=None, metavar='A',
                        help='--region_graph: adjacent regions per region, by shared boundary length (default 8, 0 .. 16; K + A 1 .. 32)')
    parser.add_argument('--rg_alpha', type=float, default=None, metavar='a',
                        help='--region_graph: the share a region takes from its neighbours per iteration (default 0.5, 0 <= a < 1)')
    parser.add_argument('--rg_gamma', type=int, default=None, metavar='G', help='--region_graph: an edge weighs similarity^G (default 3, 1 .. 8)')
    parser.add_argument('--rg_iters', type=int, default=None, metavar='T', help='--region_graph: iterations (default 20, 1 .. 10000)')
    parser.add_argument('--rg_net', type=int, default=None, metavar='I',
                        help='--region_graph: the member whose embedding describes the regions (default 0, the first)')


def region_graph_of(args, members=None):
    """the ``cmlpl_amd.regiongraph.RegionGraph`` of the command line, or None without ``--region_graph``; what it cannot mean
    is a SystemExit before anything is loaded.  ``members``: how many networks predict together (``--rg_net`` names one)"""
    given = [k for k in RG_FLAGS[1:] if getattr(args, k, None) is not None]
    if getattr(args, 'region_graph', None) is None:
        if given:
            raise SystemExit("%s belong%s to --region_graph" % (" / ".join("--" + k for k in given), "s" if len(given) == 1 else ""))
        return None
    if getattr(args, 'superpixel', None) is None:
        raise SystemExit("--region_graph belongs to --superpixel S: its nodes are the regions that vote")
    from cmlpl_amd.regiongraph import RegionGraph
    cfg = RegionGraph(**{'adj' if k == 'rg_adj' else k[3:]: getattr(args, k) for k in given})
    try:
        cfg.check(members)
    except ValueError as e:
        raise SystemExit("--region_graph: %s" % str(e).replace("RegionGraph: ", ""))
    return cfg


def load_data(run, args):
    if args.synthetic:
        run.shape = shape = SYNTH[args.synthetic]
        # (--windows cube / --synthetic_scene: both splits are seeded pixels of ONE synthetic scene, the evaluation's)
        run.from_scene = args.windows == 'cube' or args.synthetic_scene
        if run.from_scene or not args.no_eval or args.eval_every > 0 or args.knn is not None or getattr(args, 'propagate', False):
            run.whole = SyntheticScene(shape, 64, 64, seed=3)       # a 64 x 64 scene cube, every pixel a test pixel
        scene = run.whole if run.from_scene else None
        run.labeled = SyntheticHSIDataSet(shape, args.num_unlabel, 'label', seed=1, scene=scene)
        run.unlabeled = SyntheticHSIDataSet(shape, args.num_unlabel, 'unlabel', seed=2, scene=scene)
        if not args.no_eval:
            run.Y_test, run.test_array = run.whole.Y.numpy(), np.arange(len(run.whole))
    else:
        num_classes, num_features = DATASETS[int(args.dataID)]
        run.labeled = labeled = HSIDataSet(int(args.dataID), 'label', max_iters=args.num_unlabel)
        run.unlabeled = HSIDataSet(int(args.dataID), 'unlabel', max_iters=args.num_unlabel, num_unlabel=args.num_unlabel)
        if not args.no_eval:
            run.whole = HSIDataSet(int(args.dataID), 'wholeset')
            run.test_array = np.load(labeled.root + 'test_array.npy')
            run.Y_test = (np.load(labeled.root + 'Y.npy') - 1)[run.test_array]
        run.shape = (labeled.XP.shape[1], labeled.XP.shape[2], labeled.XP.shape[3], num_features, num_classes)


def build_engine(run, args, make_engine):
    world, device, bt, btu, ppb = run.world, run.device, run.bt, run.btu, args.print_per_batches
    run.hp = hp = HyperParams(lr=args.lr, num_epochs=args.num_epochs, thr=args.thr, alpha=args.alpha, queue_batch=args.queue_batch,
                              temperature=args.temperature, dropout=args.dropout, noise=args.noise)
    if world > 1 and (bt % world or btu % world):
        raise SystemExit(f"--labeled_batch_size {bt} / --unlabeled_batch_size {btu} must be multiples of the "
                         f"number of GPUs ({world}): the batch is sharded equally by sample")
    # the optimiser options: the schedule runs over the steps of the whole run, known from the splits' sizes (train.py:134)
    run.total_steps = args.num_epochs * min(-(-len(run.labeled) // bt), -(-len(run.unlabeled) // btu))
    run.optim = optim_of(args, run.total_steps)
    if make_engine is not None:
        run.eng = make_engine(NetShape(*run.shape), bt // world, btu // world, hp, ppb)
    elif world > 1:
        from cmlpl_amd.distributed import DistTrainEngine, init_distributed
        init_distributed("nccl", device)             # checked start-up: one device per local rank, no silent hang
        run.eng = DistTrainEngine(NetShape(*run.shape), bt // world, btu // world, hp, device=device, seed=1088, hist_rows=ppb)
    else:
        from cmlpl_amd import TrainEngine
        spatial = {} if args.aug_spatial == "none" else dict(aug_spatial=args.aug_spatial)
        monitor = dict(pl_monitor=True) if args.pl_stats else {}
        optim = dict(optim=run.optim) if run.optim is not None else {}
        run.eng = TrainEngine(NetShape(*run.shape), bt, btu, hp, device=device, seed=1088, hist_rows=ppb, method=args.method,
                              teacher_alpha=args.teacher_alpha if args.ema else None, **spatial, **monitor, **optim)
    run.eng.init_params_default(1088)


def open_resume(run, args):
    # every rank reads the same file (the state is replicated); what the file was trained with must be what this
    # run would train with -- the engine checks its own identity record, the flags are compared here
    run.resumed = resumed = checkpoint.load(args.resume)
    file_method = checkpoint.identity_method(resumed["identity"])
    if file_method != args.method:
        raise SystemExit("--resume %s: the file was written by --method %s, this run is --method %s" %
                         (args.resume, file_method, args.method))
    file_spatial = resumed["identity"].get("aug_spatial", "none")
    if file_spatial != args.aug_spatial:
        raise SystemExit("--resume %s: the file was written by --aug_spatial %s, this run is --aug_spatial %s" %
                         (args.resume, file_spatial, args.aug_spatial))
    diff = run_differences(resumed["extra"].get("run", {}), run_record(args, run.hp, run.shape, run.from_scene))
    if diff:
        raise SystemExit("--resume %s: this run differs from the one that wrote the file -- %s" % (args.resume, "; ".join(diff)))
    try:
        run.eng.load_checkpoint_state(resumed)
    except ValueError as e:
        raise SystemExit("--resume %s: %s" % (args.resume, e))
    run.gen.set_state(resumed["extra"]["gen_state"])


def build_loaders(run, args):
    device, labeled, unlabeled = run.device, run.labeled, run.unlabeled
    if args.windows == 'cube':
        # the scene goes to the GPU ONCE; a split is its spectra, labels and one scene pixel per row -- no windows
        if not getattr(run.eng, "takes_cube", False):
            raise SystemExit("--windows cube: this engine has no cube-fed step")
        if labeled.scene_cube is None or unlabeled.scene_cube is None:
            raise SystemExit("--windows cube needs cube.npy + scene.json in the dataset directory (sample_generation.py)")
        cube_dev = torch.from_numpy(np.ascontiguousarray(labeled.scene_cube, dtype=np.float32)).to(device)
        (Xl_, Yl_, lab_pix), (Xu_, Yu_, unl_pix) = labeled.scene_arrays(device), unlabeled.scene_arrays(device)
        lab_arrays, unl_arrays = (None, Xl_, Yl_), (None, Xu_, Yu_)
        run.cube_kw = dict(cube=cube_dev, lab_pix=lab_pix, unl_pix=unl_pix)
    else:
        lab_arrays, unl_arrays = labeled.device_arrays(device), unlabeled.device_arrays(device)
    run.lab_loader, run.unl_loader = DeviceLoader(lab_arrays, run.bt, run.gen), DeviceLoader(unl_arrays, run.btu, run.gen)
    run.num_batches = min(len(run.lab_loader), len(run.unl_loader))  # train.py:134
    run.loss_hist = np.zeros((args.num_epochs * run.num_batches, 5))  # train.py:135-136
    if run.optim is not None:         # one row per step: lr, norm, norm1, coef, coef1 (--save_optim, the optim line)
        assert run.total_steps == args.num_epochs * run.num_batches
        run.optim_hist = np.zeros((run.total_steps, 5), np.float32)


def build_evaluator(run, args):
    # the test split registered once: its pixels, spectra and labels beside the resident cube (rank 0 evaluates, as
    # after the last epoch; its own generators: no draw of the training streams is consumed)
    from cmlpl_amd.evaluate import Evaluator
    device, whole, cube_fed = run.device, run.whole, args.windows == 'cube'
    if args.synthetic:
        cube_ev = run.cube_kw["cube"] if cube_fed else whole.cube.to(device).contiguous()
        Xt, Yt = whole.X.to(device).contiguous(), whole.Y.to(device).contiguous()
        pix_t = torch.arange(len(whole), dtype=torch.int64, device=device)
    else:
        test_split = HSIDataSet(int(args.dataID), 'test')
        if test_split.scene_cube is None:
            raise SystemExit("--eval_every needs cube.npy + scene.json in the dataset directory (sample_generation.py)")
        cube_ev = run.cube_kw["cube"] if cube_fed else \
            torch.from_numpy(np.ascontiguousarray(test_split.scene_cube, dtype=np.float32)).to(device)
        Xt, Yt, pix_t = test_split.scene_arrays(device)
    run.evaluator = Evaluator(NetShape(*run.shape), cube_ev, Xt, Yt, pix_t)


def build_knn(run, args):
    """--knn: the kNN evaluation of the spectral embedding (cmlpl_amd.knn.KnnEvaluator), registered once -- the gallery is the
    labelled training pixels UNTILED (5 per class: fewer candidates of a class than k is the normal case), the queries are
    the test split's; spectra and labels only, no cube"""
    from cmlpl_amd.knn import KnnEvaluator
    if args.synthetic:
        gallery, queries = run.labeled, run.whole
    else:
        gallery, queries = HSIDataSet(int(args.dataID), 'label'), HSIDataSet(int(args.dataID), 'test')
    arrays = ((gallery.X, torch.float32), (gallery.Y, torch.int64), (queries.X, torch.float32), (queries.Y, torch.int64))
    run.knn = KnnEvaluator(NetShape(*run.shape), *(on_device(a, dt, run.device) for a, dt in arrays), k=args.knn,
                           T=args.temperature if args.knn_T is None else args.knn_T)


def build_lp(run, args):
    """--propagate: the nodes, registered once -- the labelled training pixels (the seeds: what --knn's gallery is) followed
    by the test split's pixels; spectra and labels only, no cube"""
    if args.synthetic:
        seeds, queries = run.labeled, run.whole
    else:
        seeds, queries = HSIDataSet(int(args.dataID), 'label'), HSIDataSet(int(args.dataID), 'test')
    run.lp_nodes = propagate_nodes(seeds.X, seeds.Y, queries.X, run.device)
    run.lp_truth = np.asarray(queries.Y.cpu() if torch.is_tensor(queries.Y) else queries.Y, np.int64)


def lp_lines(run, args, epoch):
    """the ``validation_lp`` / ``validation_lp1`` lines of the engine's two networks after ``epoch`` epochs; a test pixel the
    seeds do not reach counts as wrong"""
    from cmlpl_amd.labelprop import propagate_embedding, score_labels
    first = len(run.lp_nodes[1]) - len(run.lp_truth)
    with torch.no_grad():
        pairs = propagate_embedding((run.eng, None), *run.lp_nodes, run.shape[4], run.lp, probs=False)
    for net, (_, res) in enumerate(pairs):
        OA, Kappa, _, AA, _ = score_labels(res.labels[first:].cpu().numpy(), run.lp_truth, run.shape[4])
        print('Epoch %d/%d: validation_lp%s OA = %.2f AA = %.2f Kappa = %.2f' %
              (epoch, args.num_epochs, NET_TAGS[net], OA * 100, AA * 100, Kappa * 100))


def knn_lines(run, args, epoch):
    """the ``validation_knn`` / ``validation_knn1`` lines of the engine's two networks after ``epoch`` epochs: (rows, matrices)"""
    from cmlpl_amd.evaluate import metrics
    cms, rows = run.knn.evaluate((run.eng, None)).cpu().numpy(), []
    for net, cm in enumerate(cms):
        OA, Kappa, _, AA = metrics(cm)
        rows.append((OA, AA, Kappa))
        print('Epoch %d/%d: validation_knn%s OA = %.2f AA = %.2f Kappa = %.2f' %
              (epoch, args.num_epochs, NET_TAGS[net], OA * 100, AA * 100, Kappa * 100))
    return rows, cms


def restore_progress(run, args):
    ex = run.resumed["extra"]
    run.start_epoch = int(ex["epoch"])
    if ex["num_batches"] != run.num_batches or run.start_epoch > args.num_epochs:
        raise SystemExit("--resume %s: the file has %d epochs of %d steps, this run %d epochs of %d" %
                         (args.resume, run.start_epoch, ex["num_batches"], args.num_epochs, run.num_batches))
    run.loss_hist[:run.start_epoch * run.num_batches] = ex["loss_hist"].numpy()
    if run.evaluator is not None:      # (a leg without --eval_every leaves a gap in the curves, not an error)
        for curve in run.curves.values():
            curve.restore(ex)
    elif run.knn is not None:          # (--knn without --eval_every adds nothing to its curve, and keeps what it was)
        run.curves['_knn'].restore(ex)
    if args.pl_stats and "pl_curve" in ex:      # (a leg without --pl_stats leaves a gap in the curve, not an error)
        run.pl_curve = list(ex["pl_curve"].numpy())
    if run.optim is not None and "optim_hist" in ex:     # (a leg without --save_optim leaves its rows zero, not an error)
        run.optim_hist[:run.start_epoch * run.num_batches] = ex["optim_hist"].numpy()
    if run.curves[''].epochs:          # --save_best: network 0's best validation so far
        run.best_oa = max(row[0][0] for row in run.curves[''].rows)


def run_extra(run, args, epochs_done):
    """what this driver adds to a checkpoint written after ``epochs_done`` epochs"""
    first, *later = (curve.checkpoint_entries(run.shape[4]) for curve in run.curves.values())
    extra = dict(epoch=epochs_done, num_batches=run.num_batches,
                 loss_hist=torch.from_numpy(run.loss_hist[:epochs_done * run.num_batches].copy()), **first,
                 gen_state=run.gen.get_state(), args=saved_args(args),
                 run=run_record(args, run.hp, run.shape, run.from_scene), world=run.world)
    for entries in later:
        extra.update(entries)
    if args.pl_stats:                 # the monitor's counter block of every epoch so far, int64 [epochs][32 + 2 K K]
        size = 32 + 2 * run.shape[4] ** 2
        extra["pl_curve"] = torch.from_numpy(np.stack(run.pl_curve)) if run.pl_curve else torch.zeros(0, size, dtype=torch.int64)
    if args.save_optim and run.optim is not None:        # the per-step block so far: only a run that asks for it keeps it
        extra["optim_hist"] = torch.from_numpy(run.optim_hist[:epochs_done * run.num_batches].copy())
    return extra


def validate(run, args, epoch):
    """--eval_every after ``epoch`` epochs, between two steps (or replays), on their stream: launches + one read-back of nets x K x K integers"""
    eng, evaluator = run.eng, run.evaluator
    cms = (evaluator.evaluate((eng, None), ensemble=True) if args.ensemble else evaluator.evaluate((eng, None))).cpu().numpy()
    scored = {'': cms[:2]}                # in the order of the printed lines
    if args.ensemble:                     # the pair together: the third matrix of the same call (the averaged softmax's label)
        scored['_ens'] = cms[2]
    if args.ema:                          # the teachers: their packed weights are rebuilt here, when they are read
        scored['_ema'] = evaluator.evaluate((eng.teacher, None)).cpu().numpy()
    for suffix, cms in scored.items():
        curve, rows = run.curves[suffix], []
        for net, cm in enumerate(cms[None] if curve.nets is None else cms):
            OA, Kappa, _, AA = evaluator.metrics(cm)
            rows.append((OA, AA, Kappa))
            print('Epoch %d/%d: validation%s%s OA = %.2f AA = %.2f Kappa = %.2f' %
                  (epoch, args.num_epochs, suffix, NET_TAGS[net], OA * 100, AA * 100, Kappa * 100))
        curve.add(epoch, rows[0] if curve.nets is None else rows, cms)
    if run.knn is not None:               # --knn: the embedding's kNN vote, two more lines and a curve of its own
        run.curves['_knn'].add(epoch, *knn_lines(run, args, epoch))
    oa = run.curves[''].rows[-1][0][0]
    if args.save_best and (run.best_oa is None or oa > run.best_oa):
        # network 0's best validation so far (the first of equals): the state is copied on the device, behind
        # the step that produced it on the stream -- no synchronisation, no file until the run is over
        run.best_oa = oa
        run.best_state = eng.checkpoint_state(on_device=True, into=run.best_state)
        run.best_extra = run_extra(run, args, epoch)


def pl_line(epoch, num_epochs, c, graph_part):
    """the ``pl_stats`` line of one epoch's counters (a cmlpl_amd.plstats.PLCounts): per direction the selected rows and
    three accuracies in per cent; ``graph_part``: the edges of the pseudo-label graph and their precision behind them"""
    parts = []
    for d, tag in enumerate(('', '1')):
        parts.append('sel%s = %d/%d acc_sel%s = %.2f acc%s = %.2f acc_raw%s = %.2f' %
                     (tag, c.sel[d], c.rows[d], tag, c.acc_sel[d] * 100, tag, c.acc[d] * 100, tag, c.acc_raw[d] * 100))
    if graph_part:
        parts.append('pos = %d pos_precision = %.2f neg = %d neg_precision = %.2f' %
                     (c.pos, c.pos_precision * 100, c.neg, c.neg_precision * 100))
    return 'Epoch %d/%d: pl_stats %s' % (epoch, num_epochs, ' '.join(parts))


def replays(run, epoch, batches, after=-1):
    """what a captured step replays: (epoch, batch, this rank's offsets) of the epoch's full batches behind batch ``after``"""
    gbt, gbtu = run.bt // run.world, run.btu // run.world              # rows of a replayed step on this rank
    return [(epoch, bi, lo + run.rank * gbt, uo + run.rank * gbtu) for bi, ((lo, ls), (uo, us)) in enumerate(batches)
            if bi > after and ls == run.bt and us == run.btu]


def train_epochs(run, args):
    """the epoch loop (train.py:146-289): the steps, eager or replayed, the read-back of their logged rows and, behind an
    epoch, its validation and its checkpoint"""
    eng, world, rank, loss_hist, num_batches = run.eng, run.world, run.rank, run.loss_hist, run.num_batches
    lab_loader, unl_loader, cube_kw = run.lab_loader, run.unl_loader, run.cube_kw
    bt, btu, ppb = run.bt, run.btu, args.print_per_batches
    index_i = run.start_epoch * num_batches - 1
    pending = []                      # loss_hist rows of the steps run since the last read-back of the device ring

    def read_back():
        if pending:
            loss_hist[pending] = eng.loss_window(len(pending))
            if run.optim is not None:
                run.optim_hist[pending, 1:] = eng.norm_window(len(pending))
            pending.clear()
    by_index = getattr(eng, "takes_indices", False)
    truth_kw = dict(unl_truth=unl_loader.Y) if args.pl_stats else {}      # --pl_stats: the unlabelled split's labels
    # (a split smaller than one batch has no full batch to replay: such a run stays eager.  Several GPUs: the sharded
    #  step is replayed stage by stage, its collectives eager in between -- DistStepGraph; offsets are this rank's)
    use_graph = bool(args.graph) and by_index and hasattr(eng, "capture") and len(lab_loader.X) >= bt and len(unl_loader.X) >= btu
    graph = None
    t_start, steps_before = time.time(), eng.step_count              # (--resume: the steps of the earlier legs)
    t_warm, steps_warm = t_start, steps_before
    for epoch in range(run.start_epoch, args.num_epochs):            # train.py:146
        batches = list(zip(lab_loader, unl_loader))                  # (offset, size) pairs; draws this epoch's permutations
        if use_graph and graph is not None:
            # the whole epoch's per-step scalars go to the device table at once; full batches are replays
            graph.program(replays(run, epoch, batches))
        for batch_index, ((lo, ls), (uo, us)) in enumerate(batches):
            index_i += 1                                             # train.py:150
            if run.optim is not None: # the rate this step's update takes, as the kernels take it (float32)
                run.optim_hist[index_i, 0] = eng.lr_of(eng.adam_t + 1)
            bl, bul, r = ls, us, 0
            if world > 1:                                            # shard by sample; decided on GLOBAL sizes
                plan = shard_plan(ls, us, world)
                if plan is None:      # fewer rows than ranks: every rank skips alike (row stays zero in loss_hist)
                    continue
                bl, bul = plan
                r = rank
            if graph is not None and ls == bt and us == btu:
                graph.launch()
            elif by_index:
                eng.step(lab_loader.XP, lab_loader.X, lab_loader.Y, unl_loader.XP, unl_loader.X, epoch, batch_index,
                         lab_idx=lab_loader.perm[lo + r * bl:lo + (r + 1) * bl],
                         unl_idx=unl_loader.perm[uo + r * bul:uo + (r + 1) * bul], **cube_kw, **truth_kw)
            else:
                XPl, Xl, Yl = (t[r * bl:(r + 1) * bl].contiguous() for t in lab_loader.rows(lo, ls))
                XPu, Xu, Yu = (t[r * bul:(r + 1) * bul].contiguous() for t in unl_loader.rows(uo, us))
                eng.step(XPl, Xl, Yl, XPu, Xu, epoch, batch_index, **(dict(unl_truth=Yu) if args.pl_stats else {}))
            if use_graph and graph is None:
                # the first step ran eagerly (it sets the kernels' attributes); capture now and hand the rest of this
                # epoch's full batches to the graph
                graph = eng.capture(lab_loader.XP, lab_loader.X, lab_loader.Y, unl_loader.XP, unl_loader.X, lab_loader.perm,
                                    unl_loader.perm, bt // world, btu // world, capacity=max(num_batches, 1), **cube_kw,
                                    **truth_kw)
                rest = replays(run, epoch, batches, after=batch_index)
                if rest:
                    graph.program(rest)
            pending.append(index_i)
            if (batch_index + 1) % ppb == 0 or len(pending) == ppb:
                read_back()           # the five scalars of train.py:274-278 of those steps: one sync, not five per step
            if (batch_index + 1) % ppb == 0:                         # train.py:281-289 (means over the window)
                w = loss_hist[index_i - ppb + 1:index_i + 1]
                if rank == 0:
                    print('Epoch %d/%d:  %d/%d loss_contrast= %.2f total_loss = %.4f cls_loss = %.4f con_loss = %.4f '
                          'acc = %.2f\n' % (epoch + 1, args.num_epochs, batch_index + 1, num_batches,
                                            np.mean(w[:, 0]), np.mean(w[:, 1]), np.mean(w[:, 2]), np.mean(w[:, 3]),
                                            np.mean(w[:, 4]) * 100))
        read_back()                   # rows of the epoch's tail (num_batches % print_per_batches steps)
        if run.optim is not None:
            print(optim_line(epoch + 1, args.num_epochs, run.optim_hist[epoch * num_batches:(epoch + 1) * num_batches]))
        if args.pl_stats:             # the epoch's counters: read, zeroed for the next epoch, one line
            counts = eng.pl_counts()
            eng.pl_reset()
            run.pl_curve.append(counts.counts)
            print(pl_line(epoch + 1, args.num_epochs, counts, args.method == 'cmlpl'))
        if run.evaluator is not None and (epoch + 1) % args.eval_every == 0:
            validate(run, args, epoch + 1)
        if rank == 0 and args.save_ckpt and (epoch + 1 == args.num_epochs or
                                             (args.ckpt_every > 0 and (epoch + 1) % args.ckpt_every == 0)):
            # an epoch boundary: every row is read back, no replay is pending
            checkpoint.save(args.save_ckpt.replace('{epoch}', str(epoch + 1)), eng.checkpoint_state(), run_extra(run, args, epoch + 1))
        if epoch == run.start_epoch:  # (the read-back has drained the device) what follows runs on warm kernels
            t_warm, steps_warm = time.time(), eng.step_count
    if run.device.type == "cuda":
        torch.cuda.synchronize()
    if rank == 0:
        steps, t_end = eng.step_count, time.time()
        print('training: %d steps in %.3f s' % (steps - steps_before, t_end - t_start))
        if steps > steps_warm:        # the first epoch carries the one-time loading of the kernels
            print('after the first epoch: %d steps in %.3f s = %.4f ms/step' %
                  (steps - steps_warm, t_end - t_warm, (t_end - t_warm) / (steps - steps_warm) * 1e3))


def report(run, args):
    """rank 0 after the last epoch: the files of the run, the best epochs of its curves, the whole-scene evaluation"""
    eng, device, curves, base = run.eng, run.device, run.curves, run.curves['']
    if args.save_loss_hist:
        np.save(args.save_loss_hist, run.loss_hist)
    if args.save_optim:
        np.save(args.save_optim, run.optim_hist)
    if args.save_pl:
        np.save(args.save_pl, np.stack(run.pl_curve) if run.pl_curve else np.zeros((0, 32 + 2 * run.shape[4] ** 2), np.int64))
    if run.best_state is not None:
        checkpoint.save(args.save_best, run.best_state, run.best_extra)
    if args.report_memory and device.type == "cuda":
        print('peak device memory: %d bytes' % torch.cuda.max_memory_allocated(device))
    if base.epochs:
        for net in range(2):
            print(base.best_line(net))
        if args.ensemble and curves['_ens'].epochs:
            print(curves['_ens'].best_line())
        if args.save_eval:
            np.savez(args.save_eval, **{k: v for curve in curves.values() if curve.epochs for k, v in curve.npz_entries().items()})
    if run.knn is not None and not (curves['_knn'].epochs and curves['_knn'].epochs[-1] == args.num_epochs and run.evaluator is not None):
        knn_lines(run, args, args.num_epochs)        # (once after the last epoch: --eval_every has not just printed them)
    if run.lp is not None:
        lp_lines(run, args, args.num_epochs)         # --propagate: once after the last epoch
    if args.no_eval:
        return
    nets = [(net, eng.state_dict(net)) for net in range(2)]
    if args.ema:
        nets += [('ema%d' % net, eng.teacher.state_dict(net)) for net in range(2)]
    job = SceneJob(run.shape, run.whole, device, args.synthetic, args.dataID, args.dropout, run.test_array, run.Y_test,
                   run.cube_kw.get("cube"))
    evaluate_whole(job, nets, val_batch_size=args.val_batch_size,
                   last_eval=base.rows[-1] if base.epochs and base.epochs[-1] == args.num_epochs else None)
    # every report below is a prediction of its own, Base and Base1 together; --reliability: a Reliability<tag>: line behind each block
    score = RelScore(run.test_array, run.Y_test, device) if args.reliability and run.test_array is not None else None
    if args.ensemble:
        run_scene(job, nets[:2], ensemble_first(), first_block=PRINT, score=score)
    if args.tta:
        from cmlpl_amd.tta import TTA
        run_scene(job, nets[:2], tta_first(TTA(args.m, args.noise, spatial=args.tta_spatial)), first_block=PRINT, score=score)
    # --smooth, then --superpixel behind the smoothed block (else behind the pair's, which is not printed again)
    sv = sieve_of(args)                                              # --sieve: LAST, a temperature never moves a label
    rg = region_graph_of(args, 2)                                    # --region_graph: directly behind the vote it diffuses
    stages = ([smooth_stage(run.smooth)] if run.smooth is not None else []) + \
        ([superpixel_stage(run.sp, job, args.save_segments)] if run.sp is not None else []) + \
        ([region_graph_stage(rg)] if rg is not None else []) + \
        ([sieve_stage(sv)] if sv is not None else [])
    if stages:
        run_scene(job, nets[:2], ensemble_first(), stages, first_block=SILENT, score=score)


def check_reliability_args(args, smooth, sp=None):
    """what --reliability cannot mean, said before any device or communicator work"""
    if args.reliability and not (args.ensemble or args.tta or smooth is not None or sp is not None):
        raise SystemExit("--reliability scores the class probabilities of the end-of-run report's _ens / _tta / _smooth blocks: "
                         "it needs --ensemble, --tta or --smooth (or --superpixel, whose _sp block it scores as well)")
    if args.reliability and args.no_eval:
        raise SystemExit("--reliability belongs to the end-of-run report: not with --no_eval")


def check_spatial_args(args, world=1):
    """what --aug_spatial / --tta_spatial cannot mean, said before any device or communicator work"""
    if args.aug_spatial != "none":
        if world > 1:
            raise SystemExit(f"--aug_spatial {args.aug_spatial} runs on one GPU: the sharded step does not take it (this job "
                             f"has {world} ranks)")
        if args.windows != "cube":
            raise SystemExit(f"--aug_spatial {args.aug_spatial} needs --windows cube: the window's spatial element is applied "
                             "in the gather from the scene")
    if args.tta_spatial != "none" and not args.tta:
        raise SystemExit("--tta_spatial belongs to --tta")


def main(args, make_engine=None, device=None):
    """``make_engine`` / ``device`` are test hooks (tests/test_train_loop_gloo.py runs this loop as two gloo ranks
    on CPU around a stand-in engine); the product path leaves them None."""
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    smooth = smooth_of(args)                                        # (refused before any device or communicator work)
    sp = superpixel_of(args)
    if sp is not None and world > 1:
        raise SystemExit(f"--superpixel runs on one GPU (this job has {world} ranks)")
    if sp is not None and args.no_eval:
        raise SystemExit("--superpixel belongs to the end-of-run report: not with --no_eval")
    rg = region_graph_of(args, 2)
    if rg is not None and world > 1:
        raise SystemExit(f"--region_graph runs on one GPU (this job has {world} ranks)")
    sv = sieve_of(args)
    if sv is not None and world > 1:
        raise SystemExit(f"--sieve runs on one GPU (this job has {world} ranks)")
    if sv is not None and args.no_eval:
        raise SystemExit("--sieve belongs to the end-of-run report: not with --no_eval")
    if args.method != "cmlpl" and world > 1:      # before any device or communicator work
        raise SystemExit(f"--method {args.method} runs on one GPU: the sharded step exists for cmlpl only (this job has "
                         f"{world} ranks)")
    check_spatial_args(args, world)
    if args.ema and world > 1:
        raise SystemExit(f"--ema runs on one GPU: the sharded engine keeps no EMA teacher (this job has {world} ranks)")
    if args.pl_stats and world > 1:
        raise SystemExit(f"--pl_stats runs on one GPU: the sharded engine has no pseudo-label monitor (this job has {world} ranks)")
    if args.save_pl and not args.pl_stats:
        raise SystemExit("--save_pl belongs to --pl_stats")
    optim_on = [k for k, v in OPTIM_FLAGS.items() if k != 'save_optim' and getattr(args, k) != v]
    if optim_on and world > 1:
        raise SystemExit("--%s runs on one GPU: the sharded step has no schedule, weight decay or clipping (this job has %d "
                         "ranks)" % (optim_on[0], world))
    if args.save_optim and not optim_on:
        raise SystemExit("--save_optim belongs to --lr_schedule / --warmup_steps / --weight_decay / --clip_grad")
    check_reliability_args(args, smooth, sp)
    if args.knn is not None and world > 1:
        raise SystemExit(f"--knn runs on one GPU (this job has {world} ranks)")
    if args.knn is not None and not 1 <= args.knn <= 32:
        raise SystemExit("--knn K: 1 .. 32 neighbours")
    if args.knn_T is not None and (args.knn is None or not (0.0 < args.knn_T < float("inf"))):
        raise SystemExit("--knn_T T: a finite T > 0, with --knn K")
    lp = propagate_of(args)
    if lp is not None and world > 1:
        raise SystemExit(f"--propagate runs on one GPU (this job has {world} ranks)")
    if device is None:
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(device)
    torch.manual_seed(1088)                                         # seed_torch(), train.py:50-58
    # ``run`` is what the phases hand to one another; beside each is what it adds.  The curves: the two networks'; --ema: the same
    # of the teachers, a curve of their own; --ensemble: the pair's together.  ``gen``: the same permutations on every rank
    curves = [EvalCurve(sfx, nets) for sfx, nets, on in (('', 2, True), ('_ema', 2, args.ema), ('_ens', None, args.ensemble),
                                                                 ('_knn', 2, args.knn is not None)) if on]
    run = argparse.Namespace(world=world, rank=rank, device=device, bt=args.labeled_batch_size, btu=args.unlabeled_batch_size,
                             gen=torch.Generator().manual_seed(1088), curves={curve.suffix: curve for curve in curves},
                             from_scene=False, whole=None, test_array=None, Y_test=None, resumed=None, cube_kw={},
                             evaluator=None, start_epoch=0, best_oa=None, best_state=None, best_extra=None, smooth=smooth,
                             pl_curve=[], knn=None, optim=None, optim_hist=None, total_steps=0, lp=lp, sp=sp)
    load_data(run, args)              # labeled, unlabeled, shape, from_scene; whole, test_array, Y_test if anything is evaluated
    build_engine(run, args, make_engine)      # hp; eng, this rank's engine at its default initial parameters
    if args.save_best and args.eval_every <= 0:
        raise SystemExit("--save_best keeps the best-VALIDATED epoch: it needs --eval_every")
    if args.ckpt_every > 0 and not args.save_ckpt:
        raise SystemExit("--ckpt_every needs --save_ckpt PATH")
    if args.resume:
        open_resume(run, args)        # resumed, the file: its state goes into eng and gen
    build_loaders(run, args)          # lab_loader, unl_loader, num_batches, loss_hist; --windows cube: cube_kw
    if args.pl_stats and run.unl_loader.Y is None:
        raise SystemExit("--pl_stats needs the labels of the unlabelled split")
    if args.eval_every > 0 and rank == 0:
        build_evaluator(run, args)    # evaluator
    if args.knn is not None and rank == 0:
        build_knn(run, args)          # knn: --knn's gallery and queries
    if lp is not None and rank == 0:
        build_lp(run, args)           # lp_nodes, lp_truth: --propagate's seeds and test pixels
    if args.resume:
        restore_progress(run, args)   # start_epoch, its rows of loss_hist, the curves so far and best_oa
    train_epochs(run, args)
    if rank == 0:
        report(run, args)
    if world > 1 and make_engine is None:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return run.loss_hist


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--dataID', type=int, default=1)
    parser.add_argument('--num_label', type=int, default=5)
    parser.add_argument('--save_path_prefix', type=str, default='./')
    # train
    parser.add_argument('--labeled_batch_size', type=int, default=128)
    parser.add_argument('--unlabeled_batch_size', type=int, default=128)
    parser.add_argument('--val_batch_size', type=int, default=512)
    parser.add_argument('--num_workers', type=int, default=1)
    parser.add_argument('--lr', type=float, default=5e-4)
    parser.add_argument('--num_epochs', type=int, default=20)
    parser.add_argument('--print_per_batches', type=int, default=10)
    parser.add_argument('--num_unlabel', type=int, default=10000)
    parser.add_argument('--thr', type=float, default=1, help='pseudo label threshold')
    parser.add_argument('--alpha', type=float, default=0.95)
    parser.add_argument('--queue-batch', type=float, default=17, help='number of batches stored in memory bank')
    parser.add_argument('--temperature', default=0.3, type=float, help='softmax temperature')
    # network
    parser.add_argument('--teacher_alpha', type=float, default=0.95,
                        help='--ema: the coefficient of the moving average (ignored without --ema)')
    parser.add_argument('--dropout', type=float, default=0.8)
    parser.add_argument('--noise', type=float, default=0.5)
    parser.add_argument('--m', type=int, default=5, help='number of stochastic augmentations (the views of --tta)')
    # this build
    parser.add_argument('--method', choices=('cmlpl', 'cps'), default='cmlpl',
                        help="the training method: 'cmlpl' (the reference's train.py) or 'cps', the cross-pseudo-supervision "
                             "baseline of its trian_CPS.py (labelled CE + 0.1 x each network's CE against the other's "
                             "hard label; one GPU)")
    parser.add_argument('--ema', action='store_true',
                        help="keep an exponential moving average of both networks' weights (the reference's WeightEMA_BN, "
                             "coefficient --teacher_alpha), updated on the device behind every step; --eval_every scores it "
                             "too, checkpoints carry it as \"Teacher\" / \"Teacher1\" (one GPU)")
    parser.add_argument('--ensemble', action='store_true',
                        help="score the two networks TOGETHER as well: the label of their averaged softmax, on the device -- a "
                             "third validation_ens line per --eval_every evaluation (curve_ens in --save_eval) and a third "
                             "Result: block (OA_ens) after the run; --save_best keeps its criterion, network 0's OA")
    parser.add_argument('--tta', action='store_true',
                        help="test-time augmentation after the run: Base and Base1 TOGETHER score the clean window and --m "
                             "noisy views (x + --noise N(0,1)) of every scene pixel, one more Result: block (OA_tta) from "
                             "the average of all their softmaxes; the run itself is untouched")
    parser.add_argument('--tta_spatial', choices=SPATIAL_MODES, default='none',
                        help="--tta: the views are also flipped ('flips': 4 elements) or flipped and rotated ('d4': 8) windows, "
                             "view t under element (t + 1) mod 4 / 8; the Result: tag becomes _tta_flips / _tta_d4")
    parser.add_argument('--aug_spatial', choices=SPATIAL_MODES, default='none',
                        help="flip ('flips') or flip-and-rotate ('d4') augmentation of the training windows: every batch row "
                             "takes one spatial element per step, the same for both networks, applied in the gather from the "
                             "scene (needs --windows cube; one GPU)")
    parser.add_argument('--pl_stats', action='store_true',
                        help="the pseudo-label monitor: score every step's targets against the truth of its unlabelled rows, on "
                             "the device (one launch behind every step), and print one pl_stats line per epoch -- the rows the "
                             "mask selects, the accuracy of their pseudo-labels, what memory-bank smoothing changed, the "
                             "precision of the graph's positive and negative edges (one GPU).  The labels of plain --synthetic "
                             "are random: it needs --synthetic_scene (or --windows cube) for meaningful numbers")
    parser.add_argument('--save_pl', default=None, metavar='PATH',
                        help='--pl_stats: write the per-epoch counter blocks as one int64 .npy [epochs][32 + 2 K K] '
                             '(cmlpl_amd.plstats.PLCounts names the fields)')
    parser.add_argument('--reliability', action='store_true',
                        help="calibration of the end-of-run report: behind every _ens / _tta / _smooth Result: block one "
                             "Reliability<tag>: line -- ECE, MCE, NLL, Brier score, mean confidence and accuracy of the block's class "
                             "probabilities over the labelled test pixels, counted on the device (cmlpl_amd.calibrate; needs "
                             "--ensemble, --tta or --smooth).  The run itself is untouched")
    parser.add_argument('--lr_schedule', choices=('constant', 'linear', 'cosine'), default='constant',
                        help="the learning rate over the run's steps: --lr throughout ('constant', the reference), or a linear / "
                             "cosine decay from --lr towards --lr_min behind --warmup_steps steps of linear warm-up (one GPU)")
    parser.add_argument('--warmup_steps', type=int, default=0, metavar='N', help='steps of linear warm-up from --lr / N to --lr')
    parser.add_argument('--lr_min', type=float, default=0.0, metavar='F', help='--lr_schedule linear | cosine: where the decay ends')
    parser.add_argument('--weight_decay', type=float, default=0.0, metavar='F',
                        help="AdamW's decoupled weight decay of every live tensor, biases included (0: none, the reference)")
    parser.add_argument('--clip_grad', type=float, default=0.0, metavar='F',
                        help="clip each network's gradient norm to F before the update (torch's clip_grad_norm_; 0: no clipping)")
    parser.add_argument('--save_optim', default=None, metavar='PATH',
                        help='with an optimiser flag on: write [num_steps][5] = lr, norm, norm1, coef, coef1 of every step as .npy')
    add_smooth_flags(parser, 'Base and Base1 together after the run')
    add_superpixel_flags(parser, 'Base and Base1 together after the run (behind --smooth when given; one GPU)')
    add_region_graph_flags(parser, 'Base and Base1 together after the run (behind --superpixel; one GPU)')
    add_sieve_flags(parser, 'Base and Base1 together after the run (one GPU)')
    parser.add_argument('--synthetic', choices=sorted(SYNTH), default=None,
                        help='run on seeded synthetic patches of this shape (datasets are not shipped)')
    parser.add_argument('--save_loss_hist', default=None, help='write loss_hist [num_steps,5] (train.py:136) as .npy')
    parser.add_argument('--no_eval', action='store_true', help='skip the whole-image inference after training')
    parser.add_argument('--graph', action='store_true',
                        help='capture the training step once as a hipGraph and replay it (several GPUs: the sharded '
                             'step as seven stage graphs, its collectives eager between them)')
    parser.add_argument('--windows', choices=('split', 'cube'), default='split',
                        help="where a step's patch windows come from: 'split' cuts every window of both splits once and "
                             "keeps them resident (2 x 960 MB at the defaults); 'cube' uploads the scene cube once and "
                             "every step gathers its windows from it (needs cube.npy + scene.json, or --synthetic)")
    parser.add_argument('--synthetic_scene', action='store_true',
                        help='--synthetic: draw both splits from one seeded synthetic scene (implied by --windows cube)')
    parser.add_argument('--eval_every', type=int, default=0,
                        help='score both networks on the test split after every N-th epoch, on the device (0: never); '
                             'real data needs cube.npy + scene.json')
    parser.add_argument('--knn', type=int, default=None, metavar='K',
                        help="score the spectral embedding itself: the weighted kNN vote (K neighbours, cmlpl_amd.knn) of the test "
                             "split's pixels over the labelled training pixels -- two more lines validation_knn / validation_knn1 per "
                             "--eval_every evaluation (curve_knn in --save_eval and the checkpoints) and once after the last epoch; "
                             "one GPU")
    parser.add_argument('--knn_T', type=float, default=None, metavar='T',
                        help='--knn: the temperature of the vote (default: --temperature, the one the similarity softmax trains under)')
    add_propagate_flags(parser, 'two lines validation_lp / validation_lp1 after the last epoch')
    parser.add_argument('--save_eval', default=None,
                        help='--eval_every: write the curve [evaluations][nets][OA, AA, Kappa], its epochs and the '
                             'confusion matrices as .npz')
    parser.add_argument('--save_ckpt', default=None, metavar='PATH',
                        help='write a checkpoint (cmlpl_amd.checkpoint: both networks, Adam state, banks, counters) after '
                             'the last epoch; {epoch} in PATH is replaced by the 1-based epoch just finished')
    parser.add_argument('--ckpt_every', type=int, default=0, metavar='N',
                        help='--save_ckpt: also after every N-th epoch (0: only the last).  A save copies the state to the '
                             'host and writes a 28 MB file: 12.8 ms at the B2 defaults on one MI355X, about the wall time '
                             'of an EPOCH there (13.5 ms) -- every epoch doubles a run, every tenth adds a tenth')
    parser.add_argument('--resume', default=None, metavar='PATH',
                        help='load a checkpoint and continue with the epoch after it, up to --num_epochs (the hyper-parameter '
                             'flags must be those of the file; --graph, --windows, --eval_every and the GPU count may differ)')
    parser.add_argument('--save_best', default=None, metavar='PATH',
                        help="--eval_every: keep the state of network 0's best-validated epoch (copied on the device when "
                             "it is scored) and write it as a checkpoint after training")
    parser.add_argument('--report_memory', action='store_true',
                        help="print the process's peak allocated device memory after the last step")
    return parser


if __name__ == '__main__':
    main(build_parser().parse_args())
