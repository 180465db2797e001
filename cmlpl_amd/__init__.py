"""cmlpl_amd -- MI355X-native implementation of the CMLPL per-step training hot path.

Public surface:
  NetShape, HyperParams ........ shape / flag records
  TrainEngine .................. the fused training step (train.py:150-278 of the reference)
  BaseNet2 ..................... drop-in nn.Module (tools/models.py:97-152 of the reference)
  ensemble_logits / _cube / _pixels ... averaged probabilities, label, confidence, entropy of 1..4 networks
  TTA, tta_cube / tta_pixels, views_of ... the same from several noisy views per pixel (test-time augmentation)
  Smooth, smooth_probs / smooth_cube ... edge-preserving spatial smoothing of the class probability maps of a scene
  Superpixel, segment, region_vote, superpixel_probs, asa, segment_host, region_vote_host ... superpixels: segment the scene,
                                 vote per region
  components, Sieve, sieve, connect_segments, cc_label_host, sieve_host ... connected regions: label the components of a
                                 map, sieve the small ones, make a segment map connected
  RegionGraph, region_graph, region_propagate, merge_lists, pool_host, adjacency_host, merge_lists_host, region_graph_host
                                 (cmlpl_amd.regiongraph.pool / .adjacency: the two steps themselves) ... the regions of a map
                                 as the nodes of a label propagation: descriptors, adjacency, merged lists, a scene map
  PLCounts, pl_stats_host ...... the pseudo-label monitor's counters (TrainEngine(pl_monitor=True)) and their definition
  Reliability, reliability, temper_probs, fit_temperature ... calibration: reliability counters, ECE, a fitted temperature
  embed, KnnEvaluator, KnnResult, knn_host (cmlpl_amd.knn.knn: the vote itself) ... kNN evaluation of the spectral embedding
  LabelProp, label_propagation, knn_graph, build_graph, propagate, labelprop_host ... label propagation over its kNN graph
  LRSchedule, OptimConfig, grad_norm_host, clip_coef_host, adamw_host ... TrainEngine(optim=): schedule, weight decay, clipping
The compute runs in libcmlpl_hip.so (hand-written gfx950 kernels, C ABI in include/cmlpl.h);
importing the package does not load it, using any op does -- and fails loudly if it is missing.
"""
from .config import HyperParams, NetShape  # noqa: F401


def __getattr__(name):
    if name == "TrainEngine":
        from .engine import TrainEngine
        return TrainEngine
    if name in ("BaseNet2", "Normalize", "WeightEMA_BN"):
        from . import models
        return getattr(models, name)
    if name in ("ensemble_logits", "ensemble_cube", "ensemble_pixels", "EnsembleResult"):
        from . import ensemble
        return getattr(ensemble, name)
    if name in ("TTA", "tta_cube", "tta_pixels", "views_of"):
        from . import tta
        return getattr(tta, name)
    if name in ("Smooth", "smooth_probs", "smooth_cube"):
        from . import smooth
        return getattr(smooth, name)
    if name in ("Superpixel", "Segments", "RegionVote", "segment", "region_vote", "superpixel_probs", "asa", "segment_host",
                "region_vote_host"):
        from . import superpixel
        return getattr(superpixel, name)
    if name in ("Components", "Sieve", "SieveResult", "components", "sieve", "connect_segments", "cc_label_host", "sieve_host",
                "connect_segments_host"):
        from . import regions
        return getattr(regions, name)
    if name in ("RegionGraph", "region_graph", "region_propagate", "merge_lists", "pool_host", "adjacency_host",
                "merge_lists_host", "region_graph_host"):
        from . import regiongraph
        return getattr(regiongraph, name)
    if name in ("PLCounts", "pl_stats_host", "pl_stats_hard_host"):
        from . import plstats
        return getattr(plstats, name)
    if name in ("Reliability", "reliability", "temper_probs", "fit_temperature", "reliability_host", "temper_host",
                "nll_temps_host"):
        from . import calibrate
        return getattr(calibrate, name)
    if name in ("embed", "KnnEvaluator", "KnnResult", "knn_host", "vote_host"):
        from . import knn
        return getattr(knn, name)
    if name in ("LabelProp", "LPGraph", "LPResult", "label_propagation", "knn_graph", "build_graph", "one_hot_seeds", "propagate",
                "labelprop_host"):
        from . import labelprop
        return getattr(labelprop, name)
    if name in ("LRSchedule", "OptimConfig", "grad_norm_host", "clip_coef_host", "adamw_host"):
        from . import optim
        return getattr(optim, name)
    raise AttributeError(name)
