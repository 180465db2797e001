"""TrainEngine: the CMLPL training step (reference train.py:150-278) on one MI355X.

Host logic only -- state ownership (flat parameter / Adam / bank buffers as torch
tensors), the bank-pointer bookkeeping of train.py:234,237, the schedule scalars of
train.py:147-148,212 -- and ONE ctypes call per step into ``cmlpl_train_step``
(libcmlpl_hip.so).  PyTorch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import weakref
from collections import OrderedDict
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .config import FEAT_DIM, HyperParams, NetShape

_CHECK_INDICES = os.environ.get("CMLPL_CHECK_INDICES", "0") not in ("", "0")

SCALAR_NAMES = ("ctr_s", "total_s", "cls_s", "con_s", "acc", "total_w", "cls_w", "con_w", "ctr_w",
                "n_mask_w", "n_mask_s", "n_pos", "n_neg")
METHODS = tuple(_lib.METHODS)       # "cmlpl" (reference train.py), "cps" (reference trian_CPS.py)
CPS_W_CROSS = 0.1                   # weight of the cross loss, the literal of trian_CPS.py:245,248


def check_method(method: str) -> str:
    if method not in _lib.METHODS:
        raise ValueError(f"method {method!r}: one of {', '.join(METHODS)}")
    return method


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk_f32(t: torch.Tensor, shape, name):
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape) or not t.is_cuda:
        raise ValueError(f"{name}: need contiguous float32 cuda tensor of shape {tuple(shape)}, "
                         f"got {t.dtype} {tuple(t.shape)} on {t.device}")


def _chk_idx(t: torch.Tensor, name: str, rows: Optional[int] = None, what: str = "") -> None:
    """an index vector as the kernels follow it (``rows``: its length, said in ``what``)"""
    if t.dtype != torch.int64 or t.dim() != 1 or not t.is_cuda or not t.is_contiguous() \
            or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{name}: need a contiguous int64 cuda vector{what}")


def check_spatial(mode: str) -> str:
    _lib.spatial_elements(mode)
    return mode


def _fill_rows(rec, XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, bt, btu, cube=None, lab_pix=None, unl_pix=None) -> None:
    """the row sources of a cmlpl_step_io or a cmlpl_batch record (the same field names): the window tensors, or
    (cube-fed) the scene and its two pixel lists; the index lists; the batch's size"""
    rec.d_xl, rec.d_labels, rec.d_xu = Xl.data_ptr(), Y.data_ptr(), Xu.data_ptr()
    if cube is None:
        rec.d_xpl, rec.d_xpu = XPl.data_ptr(), XPu.data_ptr()
        rec.d_cube, rec.d_lab_pix, rec.d_unl_pix, rec.cube_rows, rec.cube_cols = None, None, None, 0, 0
    else:
        rec.d_xpl, rec.d_xpu = None, None
        rec.d_cube, rec.d_lab_pix, rec.d_unl_pix = cube.data_ptr(), lab_pix.data_ptr(), unl_pix.data_ptr()
        rec.cube_rows, rec.cube_cols = cube.shape[0], cube.shape[1]
    rec.d_lab_idx = None if lab_idx is None else lab_idx.data_ptr()
    rec.d_unl_idx = None if unl_idx is None else unl_idx.data_ptr()
    rec.bt, rec.btu = bt, btu


def replay_counters(ptr, adam_t: int, step_count: int, Q: int, bank_step: int, hist_rows: int, method: str, k: int):
    """``TrainEngine._advance`` for k steps ahead, as the columns of a replay table: row j is what the j-th step from
    now reads -- ``step`` and ``ptr`` as they stand BEFORE it, its own 1-based ``adam_t`` and the ``hist_row`` it writes.
    Row 0 carries the pointers as they are: ptr1 follows ptr0 (train.py:234,237) only from the first advance on."""
    j = np.arange(k, dtype=np.int64)
    p = np.empty((k, 2), np.int64)
    p[:] = ptr                            # (CPS has no memory bank: its pointers stay where they are)
    if method == "cmlpl":
        p[:, 0] = (ptr[0] + j * bank_step) % Q
        p[1:, 1] = (p[1:, 0] + bank_step) % Q
    return dict(step=step_count + j, adam_t=adam_t + 1 + j, ptr=p, hist_row=(step_count + j) % hist_rows)


class Teacher:
    """The averaged weights of an engine built with ``teacher_alpha`` (``eng.teacher``), with what
    ``cmlpl_amd.infer._nets_buffers`` / ``_net_buffers`` read from an engine: ``(eng.teacher, None)`` and
    ``(eng.teacher, k)`` go where ``(eng, None)`` and ``(eng, k)`` go -- ``infer_cube``, ``infer_pixels``,
    ``Evaluator.evaluate``.  The packed fragment sets of the averaged weights are a block of their own, allocated at first
    use and rebuilt (one full ``cmlpl_pack_weights``) only when the teacher has changed since they were last built."""

    def __init__(self, eng: "TrainEngine"):
        self._eng = eng
        self._packed = None
        self._dirty = True

    cshape = property(lambda self: self._eng.cshape)
    device = property(lambda self: self._eng.device)

    @property
    def params(self) -> torch.Tensor:
        self._eng._teacher_begin()
        return self._eng.teacher_params

    @property
    def packed(self) -> torch.Tensor:
        if self._packed is None:
            self._packed = torch.zeros_like(self._eng.packed)
            self._dirty = True
        return self._packed

    def _ensure_packed(self, stream) -> None:
        eng = self._eng
        flat, packed = self.params, self.packed
        if self._dirty:
            _lib.check("cmlpl_pack_weights",
                       eng.lib.cmlpl_pack_weights(C.byref(eng.cshape), 2, _ptr(flat), eng.P, _ptr(packed), stream))
            self._dirty = False

    def state_dict(self, net: int) -> "OrderedDict[str, torch.Tensor]":
        eng = self._eng
        return OrderedDict((k, eng.view(self.params, net, k).detach().clone()) for k in eng.state_dict_keys())


class TrainEngine:
    """Both networks (Base = net 0 / "s", Base1 = net 1 / "w"), their Adam state and
    the two memory banks, resident in HBM for the whole run.

    ``labeled_batch_size`` sizes the banks exactly like train.py:138
    (``queue_size = 5 * labeled_batch_size * 2``).  Bank writes wrap modulo the bank
    size where the reference's slice-assign would raise; the pointer advance is the
    reference literal 256 (``hp.bank_step``) -- see DESIGN.md "memory bank".

    ``method="cps"``: the cross-pseudo-supervision baseline (reference trian_CPS.py) on the same two networks -- the
    step is forward -> CPS loss (one launch) -> backward -> Adam; the banks stay allocated and untouched, ``epoch`` /
    ``batch_index`` of ``step`` play no part, ``hp.w_mutual`` is set to the reference's cross-loss weight 0.1, and
    ``loss_row`` / ``loss_window`` give the reference's row ``[con, total, cls, con, acc]`` (trian_CPS.py:254-258).

    ``aug_spatial``: flip / rotate augmentation of the CUBE-FED step's windows -- "flips" (4 elements, the reference's
    ``flip``) or "d4" (8: ``flip`` after ``Random_rot``, hsi_loader.py:58-88): every batch row takes one spatial element,
    a function of (seed, step, global sample) alone and the same for both networks (``include/cmlpl.h``, "THE DEFINITION
    OF A SPATIAL ELEMENT"), applied inside the gather launch -- no window tensor exists.  Eager and captured steps, both
    methods; a split-fed step of such an engine raises.  "none" (the default): the step and a checkpoint are what they are
    without the feature.

    ``teacher_alpha``: keep an exponential moving average of both networks' weights, the reference's
    ``WeightEMA_BN(Base, Ensemble, alpha)`` (tools/models.py:155-164) applied to the whole flat parameter block -- dead
    tensors and padding too -- behind every step that applies its update: one ``cmlpl_ema_update`` launch on the step's
    stream, eager or behind a graph replay.  The average starts as a copy of the parameters, made in front of the first
    step after construction, ``load_state_dict`` or ``init_params_default`` (``teacher_reset()`` makes it on demand);
    ``eng.teacher`` (``Teacher``) is what evaluates and saves it.  None (the default): no buffer, no launch, and a
    checkpoint is byte for byte what it is without the feature.

    ``pl_monitor``: score every step's pseudo-labels against the TRUTH of its unlabelled rows (``step(..., unl_truth=)``,
    ``capture(..., unl_truth=)``: the unlabelled split's labels, indexed the way ``Xu`` is) -- one ``cmlpl_pl_stats`` launch
    (CPS: ``cmlpl_pl_stats_hard`` on the step's hard labels) on the step's stream behind every step, eager or behind a
    graph replay, adding to a block of int64 counters (include/cmlpl.h, "THE DEFINITION OF THE PSEUDO-LABEL COUNTERS"):
    ``pl_counts()`` reads it (``cmlpl_amd.plstats.PLCounts``), ``pl_reset()`` zeroes it.  The launch reads what the step has
    left in its workspace and writes only its own block: the step, captured or not, is the code it is without it.  False
    (the default): no buffer, no launch.
    """
    takes_indices = True      # step(..., lab_idx=, unl_idx=): batches as row indices into the resident splits
    takes_cube = True         # step(None, Xl, Y, None, Xu, ..., cube=, lab_pix=, unl_pix=): windows gathered from the scene
    world = 1                 # ranks the step is sharded over (DistTrainEngine: its communicator's)

    def __init__(self, shape: NetShape, labeled_batch_size: int, unlabeled_batch_size: int,
                 hp: Optional[HyperParams] = None, device="cuda:0", seed: int = 1088, bank_labeled: int = 0,
                 hist_rows: int = 1, method: str = "cmlpl", teacher_alpha: Optional[float] = None,
                 aug_spatial: str = "none", pl_monitor: bool = False, optim=None):
        self.method = check_method(method)
        # the options of the update (cmlpl_amd.optim.OptimConfig); a record with everything off is no record
        self.optim = optim if optim is not None and optim.active() else None
        self.aug_spatial = check_spatial(aug_spatial)
        if teacher_alpha is not None and not 0.0 <= float(teacher_alpha) <= 1.0:       # (a NaN fails both comparisons)
            raise ValueError(f"teacher_alpha {teacher_alpha!r}: a coefficient in [0, 1]")
        self.teacher_alpha = None if teacher_alpha is None else float(teacher_alpha)
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("cmlpl_amd.TrainEngine needs a GPU (no CPU fallback)")
        self.shape, self.hp = shape, hp or HyperParams()
        if self.method == "cps":
            self.hp = dataclasses.replace(self.hp, w_mutual=CPS_W_CROSS)
        self.device = torch.device(device)
        self.bt_max, self.btu_max = int(labeled_batch_size), int(unlabeled_batch_size)
        self.n_max = self.bt_max + self.btu_max
        self.cshape = _lib.Shape(shape.C, shape.H, shape.W, shape.bands, shape.K)
        self.layout = _lib.layout(self.cshape)
        L = self.layout
        self.P = int(L.param_total)
        # train.py:138 (bank_labeled: the GLOBAL labelled batch under data parallelism)
        self.Q = self.hp.bank_mult * (bank_labeled or self.bt_max) * 2
        if self.Q < self.n_max:
            raise ValueError("bank smaller than one batch (needs 10*bt >= bt+btu)")
        dev = self.device
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.params, self.m, self.v, self.grads = z(2, self.P), z(2, self.P), z(2, self.P), z(2, self.P)
        self.packed = z(2, int(L.packed_total))
        self.bank_feats, self.bank_probs = z(2, self.Q, FEAT_DIM), z(2, self.Q, shape.K)   # train.py:139-144
        self.ptr = [0, 0]                                                   # train.py:141,145
        # Scalars of step i land in row i % hist_rows of a device-side ring (loss_hist of train.py:136,274-278 without
        # the reference's five .item() syncs per step): the step writes its row directly, the host reads a window
        # back once per print_per_batches steps.
        self.hist_rows = max(1, int(hist_rows))
        self.scalar_hist = z(self.hist_rows, 16)
        self._cur_row = 0
        self.logits, self.feat = z(2, self.n_max, shape.K), z(2, self.n_max, FEAT_DIM)
        ws = self.lib.cmlpl_workspace_bytes(C.byref(self.cshape), 2, self.n_max, self.Q)
        if ws == 0:
            raise _lib.CmlplError("cmlpl_workspace_bytes", -2)
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=dev)
        self.adam_t = 0
        self.step_count = 0
        self.seed = int(seed)
        self._chp = self._make_hp()
        self._packed_dirty = True
        # the step's argument record is kept: what never changes (state buffers, sizes) is set once, a step writes the
        # rest -- building the record anew and re-checking the same resident tensors cost ~40 us of Python per step
        self._io = _lib.StepIO()
        self._fill_state(self._io)
        self._checked = None
        self._checked_cube = None
        self._graph = None          # weak reference to the StepGraph that has programmed replays (see step())
        self._captured = False      # a StepGraph of this engine exists: its kernels' arguments hold the seed
        self._flag_off = None       # offset of the range flag words inside a network's packed block (asked of the library)
        self._saved_flags = None    # load_checkpoint_state: flag words to OR back in behind the next full pack
        # the EMA teacher: [2][param_stride] beside the parameters; stale = to be started from them in front of the next step
        self.teacher_params = z(2, self.P) if self.teacher_alpha is not None else None
        self.teacher = Teacher(self) if self.teacher_alpha is not None else None
        self._teacher_stale = True
        # the pseudo-label monitor: int64 counts[PL_HEAD + 2 K K], added to by one launch behind every step
        self.pl_block = torch.zeros(_lib.PL_HEAD + 2 * shape.K * shape.K, dtype=torch.int64, device=dev) if pl_monitor else None
        self._pl_off = {}           # n -> byte offset of the step's targets inside the workspace (asked of the library)
        # the clipped, decayed step: a [hist_rows][4] ring of {norm0, norm1, coef0, coef1} beside the scalars' ring and the
        # fp64 partials of the gradient-norm launch; without options neither exists and the step is the call it was
        self.norm_hist = self.norm_partials = self._copt = None
        if self.optim is not None:
            self.norm_hist = z(self.hist_rows, 4)
            self.norm_partials = torch.empty(int(self.lib.cmlpl_grad_norm_partials_bytes()) // 8, dtype=torch.float64, device=dev)
            self._copt = self._make_opt(self.norm_hist.data_ptr())

    @property
    def scalars(self) -> torch.Tensor:
        """the logged row of the last step (a view of the device ring)"""
        return self.scalar_hist[self._cur_row]

    # ------------------------------------------------------------------ parameters
    def _make_hp(self) -> _lib.HParams:
        h = self.hp
        return _lib.HParams(h.lr, h.beta1, h.beta2, h.eps, h.temperature, h.alpha, h.noise, h.dropout,
                            h.w_contrast, h.w_mutual, h.pos_thr, h.neg_thr)

    # ------------------------------------------------------------------ schedule, weight decay, clipping
    def _make_opt(self, d_norms: int) -> "_lib.Optim":
        o = self.optim
        return _lib.Optim(float(o.clip_grad), float(o.weight_decay), d_norms, self.norm_partials.data_ptr())

    def lr_of(self, t: int) -> float:
        """the learning rate of the 1-based Adam step ``t`` as the kernels take it: the float32 of the schedule's
        ``lr_at(t)`` (of ``hp.lr`` without a schedule)"""
        o = self.optim
        lr = self.hp.lr if o is None or o.schedule is None else o.schedule.lr_at(t)
        return float(C.c_float(lr).value)

    def _hp_at(self, t: int) -> "_lib.HParams":
        """the step's hyper-parameter record: ``self._chp``, or a copy carrying the scheduled rate of Adam step ``t``"""
        if self.optim is None or self.optim.schedule is None:
            return self._chp
        hp = _lib.HParams.from_buffer_copy(self._chp)
        hp.lr = self.lr_of(t)
        return hp

    def grad_norms(self):
        """[norm0, norm1, coef0, coef1] of the last step (a synchronising read): each network's gradient norm and the
        clip coefficient its update used (1 without clipping)"""
        if self.norm_hist is None:
            raise RuntimeError("grad_norms(): an engine built with optim=OptimConfig(...) with an option on")
        return self.norm_hist[self._cur_row].tolist()

    def norm_window(self, k: int):
        """the norms rows of the last k steps, oldest first, float32 numpy [k][4] (as ``loss_window``; one read-back)"""
        if self.norm_hist is None:
            raise RuntimeError("norm_window(): an engine built with optim=OptimConfig(...) with an option on")
        return self._ring_rows(self.norm_hist, k).cpu().numpy()

    def tensor_shapes(self) -> "OrderedDict[str, tuple]":
        s = self.shape
        return OrderedDict([
            ("conv0.weight", (64, s.C, 1, 1)), ("conv0.bias", (64,)),
            ("conv1.weight", (64, 64, 3, 3)), ("conv1.bias", (64,)),
            ("conv2.weight", (64, 64, 3, 3)), ("conv2.bias", (64,)),
            ("feat_spe.weight", (FEAT_DIM, s.bands)), ("feat_spe.bias", (FEAT_DIM,)),
            ("classifier.weight", (s.K, s.cls_in)), ("classifier.bias", (s.K,)),
            ("feat_ss.weight", (256, FEAT_DIM)), ("feat_ss.bias", (256,)),
            ("feat_ss2.weight", (64, FEAT_DIM)), ("feat_ss2.bias", (64,)),
            ("feat_ss3.weight", (64, 256)), ("feat_ss3.bias", (64,)),
        ])

    def view(self, buf: torch.Tensor, net: int, key: str) -> torch.Tensor:
        i = _lib.TENSOR_KEYS.index(key)
        off, numel = int(self.layout.param_off[i]), int(self.layout.param_numel[i])
        return buf[net, off:off + numel].view(self.tensor_shapes()[key])

    def load_state_dict(self, net: int, sd: Dict[str, torch.Tensor]) -> None:
        for key in _lib.TENSOR_KEYS:
            if key in sd:
                self.view(self.params, net, key).copy_(sd[key].to(self.device, torch.float32))
        self._packed_dirty = True
        self._teacher_stale = True

    def state_dict(self, net: int) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((k, self.view(self.params, net, k).detach().clone()) for k in self.state_dict_keys())

    def grad(self, net: int, key: str) -> torch.Tensor:
        return self.view(self.grads, net, key)

    def init_params_default(self, seed: int = 1088) -> None:
        """torch default init of nn.Conv2d / nn.Linear (kaiming-uniform a=sqrt(5)):
        U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and bias."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        shapes = self.tensor_shapes()
        for net in range(2):
            for key, shp in shapes.items():
                fan_in = 1
                for d in shapes[key.split(".")[0] + ".weight"][1:]:
                    fan_in *= d
                b = 1.0 / (fan_in ** 0.5)
                self.view(self.params, net, key).copy_((torch.rand(shp, generator=g) * 2 - 1) * b)
        self._packed_dirty = True
        self._teacher_stale = True

    # ------------------------------------------------------------------ the EMA teacher
    def teacher_reset(self) -> None:
        """the teacher := the parameters as they are now (stream-ordered device copy)"""
        if self.teacher is None:
            raise RuntimeError("teacher_reset(): an engine built with teacher_alpha")
        self.teacher_params.copy_(self.params)
        self.teacher._dirty = True
        self._teacher_stale = False

    def _teacher_begin(self) -> None:
        if self.teacher is not None and self._teacher_stale:
            self.teacher_reset()

    def _teacher_update(self, stream) -> None:
        """behind a step that has applied its update: teacher = params * (1 - alpha) + teacher * alpha over the whole block"""
        _lib.check("cmlpl_ema_update", self.lib.cmlpl_ema_update(_ptr(self.params), _ptr(self.teacher_params),
                                                                 2 * self.P, self.teacher_alpha, stream))
        self.teacher._dirty = True

    # ------------------------------------------------------------------ the pseudo-label monitor
    def _pl_truth(self, unl_truth, rows: int) -> torch.Tensor:
        if unl_truth is None:
            raise ValueError("an engine built with pl_monitor scores every step: pass unl_truth (the unlabelled rows' labels)")
        _chk_idx(unl_truth, "unl_truth", rows, f", one label per unlabelled row ({rows})")
        return unl_truth

    def _pl_update(self, stream, truth: torch.Tensor, idx_ptr, btu: int, adap_mask: float) -> None:
        """behind a step of ``self._last_n`` rows: its targets, still in the workspace, against ``truth`` (read at
        ``idx_ptr[r]``, or at r); ``adap_mask``: the float32 value that step compared with"""
        n, K = self._last_n, self.shape.K
        region = "probs" if self.method == "cmlpl" else "cps_pseudo"
        if n not in self._pl_off:
            off, nbytes = C.c_size_t(), C.c_size_t()
            _lib.check("cmlpl_debug_region", self.lib.cmlpl_debug_region(
                C.byref(self.cshape), 2, n, region.encode(), C.byref(off), C.byref(nbytes)))
            self._pl_off[n] = int(off.value)
        src = C.c_void_p(self.workspace.data_ptr() + self._pl_off[n])
        if self.method == "cmlpl":
            _lib.check("cmlpl_pl_stats", self.lib.cmlpl_pl_stats(
                src, btu, K, _ptr(truth), idx_ptr, adap_mask, self._chp.pos_thr, self._chp.neg_thr, _ptr(self.pl_block), stream))
        else:
            _lib.check("cmlpl_pl_stats_hard", self.lib.cmlpl_pl_stats_hard(src, btu, K, _ptr(truth), idx_ptr,
                                                                           _ptr(self.pl_block), stream))

    def pl_counts(self):
        """the counters since the last ``pl_reset()`` as a ``cmlpl_amd.plstats.PLCounts`` (a synchronising read)"""
        if self.pl_block is None:
            raise RuntimeError("pl_counts(): an engine built with pl_monitor")
        from .plstats import PLCounts
        return PLCounts(self.pl_block.cpu().numpy(), self.shape.K)

    def pl_reset(self) -> None:
        """zero the counters (a stream-ordered memset: behind every launch enqueued so far)"""
        if self.pl_block is None:
            raise RuntimeError("pl_reset(): an engine built with pl_monitor")
        self.pl_block.zero_()

    def _ensure_packed(self, stream) -> None:
        if self._packed_dirty:
            _lib.check("cmlpl_pack_weights",
                       self.lib.cmlpl_pack_weights(C.byref(self.cshape), 2, _ptr(self.params), self.P,
                                                   _ptr(self.packed), stream))
            self._packed_dirty = False
            if self._saved_flags is not None:
                # the full pack after load_checkpoint_state: it has just set the range flag words anew from the current
                # weights; a flag the saved run had raised earlier (sticky until a full pack) is OR-ed back in
                self._flag_words().bitwise_or_(self._saved_flags)
                self._saved_flags = None

    # ------------------------------------------------------------------ checkpoints (cmlpl_amd/checkpoint.py)
    def _flag_words(self) -> torch.Tensor:
        """the two-piece range flag words of both networks, [2][16] int32: a view of the tail of ``packed``"""
        if self._flag_off is None:
            off = C.c_int64()
            _lib.check("cmlpl_packed_flag_offset", self.lib.cmlpl_packed_flag_offset(C.byref(self.cshape), C.byref(off)))
            self._flag_off = int(off.value)
        return self.packed[:, self._flag_off:].view(torch.int32)

    def _refuse_pending(self, what: str, or_else: str = "") -> None:
        g = self._graph() if self._graph is not None else None
        if g is not None and g.pending > 0:
            # the programmed rows were formed from counters and bank pointers the replays have yet to catch up with
            raise RuntimeError(f"{g.pending} programmed graph replays are pending: launch them{or_else} before {what}")

    def identity(self) -> Dict[str, object]:
        """what a checkpoint must agree with to be loaded here (batch capacities GLOBAL: a sharded engine's are per rank)"""
        from .checkpoint import make_identity
        return make_identity(self.shape, self.hp, self.bt_max * self.world, self.btu_max * self.world, self.Q,
                             self.lib.cmlpl_source_hash().decode(), _lib.ABI_VERSION, method=self.method,
                             teacher_alpha=self.teacher_alpha, aug_spatial=self.aug_spatial, optim=self.optim)

    def checkpoint_state(self, on_device: bool = False, into: Optional[dict] = None) -> dict:
        """Everything the step carries from one step to the next (``grads``, the workspace and the logging ring are
        scratch; ``packed`` is derived, but for its range flag words), as a dict of tensors and plain values --
        ``cmlpl_amd.checkpoint.save`` writes it, ``load_checkpoint_state`` takes it back.  Host copies by default (one
        synchronisation); ``on_device``: stream-ordered device copies and NO synchronisation (train.py --save_best keeps
        the best-validated state this way), into the tensors of ``into`` -- an earlier on-device state of this engine --
        when given.  Raises while programmed graph replays are pending."""
        self._refuse_pending("checkpoint_state()")
        self._ensure_packed(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))   # (flag words of THESE weights)
        src = dict(params=self.params, m=self.m, v=self.v, bank_feats=self.bank_feats, bank_probs=self.bank_probs,
                   range_flags=self._flag_words())
        for net, key in enumerate(("Base", "Base1")):
            src[key] = OrderedDict((k, self.view(self.params, net, k)) for k in self.state_dict_keys())
        if self.teacher is not None:
            self._teacher_begin()
            src["teacher_params"] = self.teacher_params
            for net, key in enumerate(("Teacher", "Teacher1")):
                src[key] = OrderedDict((k, self.view(self.teacher_params, net, k)) for k in self.state_dict_keys())
        if into is not None:
            st = into
            for k, t in src.items():
                if isinstance(t, dict):
                    for kk, tt in t.items():
                        st[k][kk].copy_(tt)
                else:
                    st[k].copy_(t)
        else:
            take = (lambda t: t.detach().clone()) if on_device else (lambda t: t.detach().cpu())
            st = {k: (OrderedDict((kk, take(tt)) for kk, tt in t.items()) if isinstance(t, dict) else take(t))
                  for k, t in src.items()}
        st.update(ptr=[int(self.ptr[0]), int(self.ptr[1])], adam_t=int(self.adam_t), step_count=int(self.step_count),
                  seed=int(self.seed), identity=self.identity())
        return st

    def load_checkpoint_state(self, state: dict) -> None:
        """Continue from ``state`` (``checkpoint_state()``, or a file through ``cmlpl_amd.checkpoint.load``): copied INTO
        the engine's tensors (a captured graph holds their addresses).  ValueError naming every field of the identity
        record that differs (``cmlpl_amd.checkpoint.check_identity``).  The packed weights are rebuilt by the next step's
        full pack, behind which the saved range flag words are OR-ed back in.  Raises while replays are pending."""
        from .checkpoint import check_identity
        self._refuse_pending("load_checkpoint_state()")
        check_identity(state["identity"], self.identity())
        flags = state["range_flags"]
        if tuple(flags.shape) != tuple(self._flag_words().shape) or flags.dtype != torch.int32:
            raise ValueError(f"range_flags: need int32 {tuple(self._flag_words().shape)}, the checkpoint has "
                             f"{flags.dtype} {tuple(flags.shape)}")
        for name in ("params", "m", "v", "bank_feats", "bank_probs"):
            dst, t = getattr(self, name), state[name]
            if tuple(t.shape) != tuple(dst.shape) or t.dtype != dst.dtype:
                raise ValueError(f"{name}: need {dst.dtype} {tuple(dst.shape)}, the checkpoint has {t.dtype} {tuple(t.shape)}")
        for name in ("params", "m", "v", "bank_feats", "bank_probs"):
            getattr(self, name).copy_(state[name])
        self.ptr = [int(state["ptr"][0]), int(state["ptr"][1])]
        if int(state["seed"]) != self.seed:
            if self._captured:
                raise ValueError(f"seed: file {int(state['seed'])}, here {self.seed} -- and a step of this engine has been "
                                 "captured with its own (load before capturing, or construct the engine with the file's seed)")
            self.seed = int(state["seed"])
            self._set_seed()
        self.adam_t, self.step_count = int(state["adam_t"]), int(state["step_count"])
        self._saved_flags = flags.to(self.device).clone()
        self._packed_dirty = True
        if self.teacher is not None:
            # (a state without a teacher: the average starts from the loaded parameters; an engine without one ignores
            #  the state's)
            t = state.get("teacher_params")
            if t is None:
                self.teacher_reset()
            else:
                if tuple(t.shape) != tuple(self.teacher_params.shape) or t.dtype != torch.float32:
                    raise ValueError(f"teacher_params: need float32 {tuple(self.teacher_params.shape)}, the checkpoint has "
                                     f"{t.dtype} {tuple(t.shape)}")
                self.teacher_params.copy_(t)
                self.teacher._dirty = True
                self._teacher_stale = False

    def _set_seed(self) -> None:
        self._io.seed = self.seed

    def state_dict_keys(self):
        """the 16 keys in the registration order of tools/models.py:102-127"""
        order = ["conv0", "conv1", "conv2", "feat_spe", "feat_ss", "feat_ss2", "feat_ss3", "classifier"]
        return [f"{mod}.{leaf}" for mod in order for leaf in ("weight", "bias")]

    # ------------------------------------------------------------------ the step
    def _check_batch(self, XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, cube, lab_pix, unl_pix):
        """The check of a batch, eager or captured -> (bt, btu).  Split-fed: the rows themselves, or (lab_idx / unl_idx
        given) the resident splits the index lists point into (hsi_loader.py:109-133 hands rows out by index; here the
        kernels follow the index).  CUBE-FED (any of cube / lab_pix / unl_pix given): the scene [rows][cols][C], the spectra /
        labels of the splits (or of the batch), one scene pixel per split row and no window tensors."""
        s = self.shape
        cube_fed = cube is not None or lab_pix is not None or unl_pix is not None
        if cube_fed:
            if XPl is not None or XPu is not None:
                raise ValueError("a cube-fed step takes no window tensors: pass XPl = XPu = None")
            if cube is None or lab_pix is None or unl_pix is None:
                raise ValueError("a cube-fed step needs cube, lab_pix and unl_pix")
            key = (id(cube), id(Xl), id(Y), id(Xu), id(lab_pix), id(unl_pix), cube.data_ptr(), lab_pix.data_ptr(),
                   unl_pix.data_ptr(), tuple(cube.shape), Xl.shape[0], Xu.shape[0])
            if key != self._checked_cube:         # another scene than last time
                self._check_scene(cube, Xl, Y, Xu, lab_pix, unl_pix)
                self._checked_cube = key
            nl, nu = Xl.shape[0], Xu.shape[0]
        else:
            if self.aug_spatial != "none":
                self._refuse_split_fed()
            if lab_idx is not None and unl_idx is not None:
                # the same resident splits as last time (by identity and storage): only the index lists are new
                key = (id(XPl), id(Xl), id(Y), id(XPu), id(Xu), XPl.data_ptr(), XPu.data_ptr(), XPl.shape[0], XPu.shape[0])
                if key == self._checked and lab_idx.dtype == torch.int64 and unl_idx.dtype == torch.int64 \
                        and lab_idx.is_cuda and unl_idx.is_cuda and lab_idx.dim() == 1 and unl_idx.dim() == 1 \
                        and lab_idx.is_contiguous() and unl_idx.is_contiguous():
                    bt, btu = lab_idx.shape[0], unl_idx.shape[0]
                    if 1 <= bt <= self.bt_max and btu >= 1 and bt + btu <= self.n_max:
                        return bt, btu
            nl, nu = XPl.shape[0], XPu.shape[0]
        if (lab_idx is None) != (unl_idx is None):
            raise ValueError("lab_idx and unl_idx come together")
        if lab_idx is not None:
            _chk_idx(lab_idx, "lab_idx")
            _chk_idx(unl_idx, "unl_idx")
        bt = nl if lab_idx is None else lab_idx.shape[0]
        btu = nu if unl_idx is None else unl_idx.shape[0]
        if bt < 1 or btu < 1 or bt > self.bt_max or bt + btu > self.n_max:
            raise ValueError(f"batch {bt}+{btu} outside the engine's capacity {self.bt_max}+{self.btu_max}")
        if not cube_fed:
            _chk_f32(XPl, (nl, s.C, s.H, s.W), "XPl"); _chk_f32(XPu, (nu, s.C, s.H, s.W), "XPu")
            self._check_spectra(Xl, Y, Xu)
            if lab_idx is not None:
                self._checked = key
        return bt, btu

    def _check_spectra(self, Xl, Y, Xu) -> None:
        nl, bands = Xl.shape[0], self.shape.bands
        _chk_f32(Xl, (nl, bands), "Xl"); _chk_f32(Xu, (Xu.shape[0], bands), "Xu")
        if Y.dtype != torch.int64 or tuple(Y.shape) != (nl,) or not Y.is_cuda:
            raise ValueError("Y: need int64 cuda tensor, one label per labelled row")

    def _check_scene(self, cube, Xl, Y, Xu, lab_pix, unl_pix) -> None:
        """The resident arrays of a cube-fed batch.  The pixel lists are range-checked here ONCE per array (a
        synchronising min / max; the gather follows them without a bounds check), not per step."""
        s = self.shape
        if s.H != s.W:
            raise ValueError(f"cube-fed windows are square, the shape has {s.H} x {s.W}")
        if cube.dim() != 3 or cube.dtype != torch.float32 or not cube.is_contiguous() or not cube.is_cuda:
            raise ValueError("cube: need a contiguous float32 cuda tensor [rows][cols][C]")
        rows, cols, ch = cube.shape
        if ch != s.C:
            raise ValueError(f"cube: {ch} channels, the shape has C = {s.C}")
        if rows < s.H or cols < s.W:
            raise ValueError(f"cube: scene {rows} x {cols} smaller than the {s.H} x {s.W} window")
        self._check_spectra(Xl, Y, Xu)
        for name, t, n in (("lab_pix", lab_pix, Xl.shape[0]), ("unl_pix", unl_pix, Xu.shape[0])):
            _chk_idx(t, name, n, f", one scene pixel per split row ({n})")
            self.check_index_range(t, rows * cols, name)

    @staticmethod
    def check_index_range(idx: torch.Tensor, rows: int, name: str = "index") -> None:
        """Every entry of an index list inside [0, rows): the kernels follow the indices without a bounds check, so a
        stale or corrupt permutation would be an out-of-bounds device read.  One synchronising min / max: call it
        where a list is FILLED (the loader's per-epoch permutation, StepGraph's buffers), not per step;
        ``CMLPL_CHECK_INDICES=1`` makes ``step()`` call it on every batch (bring-up only)."""
        if idx.numel() == 0:
            return
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= rows:
            raise ValueError(f"{name}: entries span [{lo}, {hi}], the resident split has {rows} rows")

    _fill_io = staticmethod(_fill_rows)       # (io, XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, bt, btu, cube, lab_pix, unl_pix)

    def _fill_banks(self, b) -> None:
        """what never changes of a cmlpl_banks record (its two pointers follow ``self.ptr`` step by step)"""
        for i in range(2):
            b.d_feats[i] = self.bank_feats[i].data_ptr()
            b.d_probs[i] = self.bank_probs[i].data_ptr()
        b.Q = self.Q

    def _fill_state(self, io):
        io.d_params, io.d_m, io.d_v = self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr()
        io.d_grads, io.d_packed = self.grads.data_ptr(), self.packed.data_ptr()
        self._fill_banks(io.banks)
        # outputs are laid out [2][n][..] for THIS n (views of the max-size buffers)
        io.d_logits, io.d_feat = self.logits.data_ptr(), self.feat.data_ptr()
        io.d_workspace, io.workspace_bytes = self.workspace.data_ptr(), self.workspace.numel()
        io.seed = self.seed
        # cmlpl_step_io.reserved: the method (0 = CMLPL) in bits 0..7, the spatial augmentation (0 = none) in bits 8..9
        io.reserved = _lib.METHODS[self.method] | (_lib.SPATIAL[self.aug_spatial] << 8)

    def _refuse_split_fed(self) -> None:
        if self.aug_spatial != "none":
            raise ValueError(f"aug_spatial={self.aug_spatial!r} needs cube-fed steps (cube=, lab_pix=, unl_pix=): the "
                             "window's spatial element is applied in the gather from the scene")

    def _advance(self, n, apply_update=True, row=None):
        """THE step bookkeeping, behind every step of n rows however it ran (eager, replayed, sharded): the ring row it
        wrote (``row``, where the caller has formed it already), bank pointers (train.py:234,237 -- ptr1 follows ptr0,
        reference quirk kept), Adam step, step counter.  ``replay_counters`` states the same rule for k steps ahead."""
        self._cur_row = self.step_count % self.hist_rows if row is None else row
        if self.method == "cmlpl":        # (CPS has no memory bank: its pointers stay where they are)
            p0 = (self.ptr[0] + self.hp.bank_step) % self.Q
            self.ptr = [p0, (p0 + self.hp.bank_step) % self.Q]
        if apply_update:
            self.adam_t += 1
        self.step_count += 1
        self._last_n = n

    def step(self, XPl: torch.Tensor, Xl: torch.Tensor, Y: torch.Tensor, XPu: torch.Tensor, Xu: torch.Tensor,
             epoch: int, batch_index: int, noise: Optional[Sequence[torch.Tensor]] = None,
             dropmask: Optional[torch.Tensor] = None, apply_update: bool = True,
             lab_idx: Optional[torch.Tensor] = None, unl_idx: Optional[torch.Tensor] = None,
             cube: Optional[torch.Tensor] = None, lab_pix: Optional[torch.Tensor] = None,
             unl_pix: Optional[torch.Tensor] = None, unl_truth: Optional[torch.Tensor] = None) -> None:
        """One training step; asynchronous.  Results land in ``self.scalars`` (device),
        ``self.logits`` / ``self.feat`` ([2][n][..]) and ``self.grads``.

        noise    : None -> in-kernel draws (PCG4D hash + Box-Muller); or the 8 draws in reference order (parity mode)
        dropmask : None -> Philox4x32-10 mask (or no dropout when hp.dropout == 0); or [2][n][cls_in] multipliers
        lab_idx / unl_idx : None -> XPl .. Xu ARE the batch; or int64 row numbers: XPl / Xl / Y (XPu / Xu) are then the
                   whole resident labelled (unlabelled) split and batch row s is its row lab_idx[s] (unl_idx[s]) --
                   no gathered copy of the batch is made (noise / dropmask stay indexed by batch row)
        cube / lab_pix / unl_pix : the CUBE-FED step -- XPl and XPu are None: no window tensor exists.  ``cube`` is the
                   resident scene [rows][cols][C]; the patch row of a batch row is the H x W window (mirror index of
                   ExtractPatches) of scene pixel lab_pix[r] (unl_pix[r]), r = the split row Xl / Y (Xu) are read at.
                   Bit-identical to the step on ``extract_patches(cube, pix)``.
        unl_truth : an engine built with ``pl_monitor`` only (others ignore it): the labels of the unlabelled rows, int64,
                   indexed the way Xu is -- the whole split's when unl_idx is given, the batch's otherwise
        """
        s = self.shape
        if self._graph is not None:
            self._refuse_pending("an eager step", " (or program() anew)")
        bt, btu = self._check_batch(XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, cube, lab_pix, unl_pix)
        if _CHECK_INDICES and lab_idx is not None:
            self.check_index_range(lab_idx, Xl.shape[0], "lab_idx")
            self.check_index_range(unl_idx, Xu.shape[0], "unl_idx")
        n = bt + btu
        if self.pl_block is not None:
            unl_truth = self._pl_truth(unl_truth, Xu.shape[0] if unl_idx is not None else btu)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._ensure_packed(stream)
        self._teacher_begin()
        io = self._io
        _fill_rows(io, XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, bt, btu, cube, lab_pix, unl_pix)
        io.noise8, io.d_dropmask = None, None
        keep = None
        if noise is not None:
            xpl, xl, xpu, xu = (bt, s.C, s.H, s.W), (bt, s.bands), (btu, s.C, s.H, s.W), (btu, s.bands)
            shp = [xpl, xl, xpl, xl, xpu, xu, xpu, xu]
            for t, sh in zip(noise, shp):
                _chk_f32(t, sh, "noise")
            keep = (C.c_void_p * 8)(*[t.data_ptr() for t in noise])
            io.noise8 = C.cast(keep, C.POINTER(C.c_void_p))
        if dropmask is not None:
            _chk_f32(dropmask, (2, n, s.cls_in), "dropmask")
            io.d_dropmask = dropmask.data_ptr()
        for i in range(2):
            io.banks.ptr[i] = self.ptr[i]
        row = self.step_count % self.hist_rows        # of the two logging rings
        io.d_scalars = self.scalar_hist.data_ptr() + 64 * row
        io.smooth = 1 if self.hp.smooth_gate(epoch, batch_index) else 0
        io.adap_mask = float(self.hp.thr * self.hp.adap_thr(epoch))        # train.py:221
        io.adam_t = self.adam_t + 1
        io.step = self.step_count
        io.apply_update = 1 if apply_update else 0
        if self.optim is None:
            _lib.check("cmlpl_train_step",
                       self.lib.cmlpl_train_step(C.byref(self.cshape), C.byref(self._chp), C.byref(io), stream))
        else:
            self._copt.d_norms = self.norm_hist.data_ptr() + 16 * row
            _lib.check("cmlpl_train_step_opt", self.lib.cmlpl_train_step_opt(
                C.byref(self.cshape), C.byref(self._hp_at(self.adam_t + 1)), C.byref(io), C.byref(self._copt), stream))
        if self.teacher is not None and apply_update:
            self._teacher_update(stream)
        self._advance(n, apply_update, row)
        self._last_btu = btu
        if self.pl_block is not None:     # one launch behind the step, on its stream; io.adap_mask: the float32 the step read
            self._pl_update(stream, unl_truth, _ptr(unl_idx), btu, io.adap_mask)

    def capture(self, XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, bt: int, btu: int, capacity: int = 1024,
                cube=None, lab_pix=None, unl_pix=None, unl_truth=None) -> "StepGraph":
        """The step captured ONCE as a hipGraph over the resident splits and two index buffers (lab_idx / unl_idx: the
        epoch's permutations, re-filled in place by the caller); see StepGraph.  Cube-fed (cube / lab_pix / unl_pix
        given, XPl = XPu = None): over the resident scene instead of the window tensors.  ``unl_truth``: the unlabelled
        split's labels, for an engine built with ``pl_monitor`` (its launch follows every replay; it is not captured)."""
        return StepGraph(self, XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, bt, btu, capacity, cube, lab_pix, unl_pix, unl_truth)

    def outputs(self):
        """(logits [2][n][K], feat [2][n][1024]) of the last step."""
        n = self._last_n
        K = self.shape.K
        lo = self.logits.view(-1)[: 2 * n * K].view(2, n, K)
        fe = self.feat.view(-1)[: 2 * n * FEAT_DIM].view(2, n, FEAT_DIM)
        return lo, fe

    def debug_region(self, name: str, dtype=torch.float32) -> torch.Tensor:
        """View of a saved activation of the last step inside the workspace (inspection / tests);
        see cmlpl_debug_region in include/cmlpl.h."""
        off, nbytes = C.c_size_t(), C.c_size_t()
        _lib.check("cmlpl_debug_region", self.lib.cmlpl_debug_region(
            C.byref(self.cshape), 2, self._last_n, name.encode(), C.byref(off), C.byref(nbytes)))
        return self.workspace[off.value: off.value + nbytes.value].view(dtype)

    def read_scalars(self) -> Dict[str, float]:
        """Synchronising read of the logged row (train.py:274-278) and friends."""
        vals = self.scalars.tolist()
        return dict(zip(SCALAR_NAMES, vals))

    def loss_row(self):
        """[loss_contrast, total_loss, cls_loss, con_loss, acc] -- loss_hist row, train.py:274-278.  CPS: the row of
        trian_CPS.py:254-258, whose column 0 repeats the cross loss."""
        row = self.scalars[:5].tolist()
        if self.method == "cps":
            row[0] = row[3]
        return row

    def pseudo_labels(self) -> torch.Tensor:
        """CPS: the hard labels of the last step, int64 [2][btu] = (Base's targets = argmax of Base1's logits, Base1's
        targets = argmax of Base's) -- a view of the workspace (trian_CPS.py:238-239)."""
        if self.method != "cps":
            raise RuntimeError("pseudo_labels(): a CPS engine's output")
        btu = self._last_btu
        return self.debug_region("cps_pseudo", torch.int64)[: 2 * btu].view(2, btu)

    def loss_window(self, k: int):
        """loss_hist[index_i-k+1 : index_i+1] (train.py:285-289) as a float64 numpy array [k,5]: the rows of the
        last k steps, oldest first.  One synchronising read-back."""
        out = self._reduce_rows(self._ring_rows(self.scalar_hist, k))[:, :5].double().cpu().numpy()
        if self.method == "cps":
            out[:, 0] = out[:, 3]          # trian_CPS.py:254: column 0 repeats the cross loss
        return out

    def _ring_rows(self, hist: torch.Tensor, k: int) -> torch.Tensor:
        """the rows that the last k steps wrote into a [hist_rows][..] ring, oldest first"""
        if k < 1 or k > self.hist_rows or k > self.step_count:
            raise ValueError(f"window of {k} steps not held (hist_rows={self.hist_rows}, steps={self.step_count})")
        idx = [(self.step_count - k + j) % self.hist_rows for j in range(k)]
        return hist[torch.tensor(idx, device=self.device)]

    def _reduce_rows(self, rows: torch.Tensor) -> torch.Tensor:
        return rows


class _ReplayTable:
    """What a captured step replays from, single-GPU (``StepGraph``) or sharded (``DistStepGraph``): the device table of
    ``cmlpl_dyn`` rows with its cursor, the pinned rows ``program()`` fills them through, and the checks of a capture's
    arguments.  What is captured, and what a replay launches, is the subclass's."""

    def __init__(self, eng: TrainEngine, XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, bt: int, btu: int, capacity: int,
                 cube, lab_pix, unl_pix, unl_truth=None, a_batch: str = "batch"):
        self.eng, self.bt, self.btu, self.capacity = eng, int(bt), int(btu), int(capacity)
        if lab_idx is None or unl_idx is None:
            raise ValueError("a captured step reads its rows through index buffers")
        if lab_idx.shape[0] < bt or unl_idx.shape[0] < btu:
            raise ValueError(f"index buffers shorter than one {a_batch}")
        # (a batch the engine does not take is refused before its tensors are looked at)
        eng._check_batch(XPl, Xl, Y, XPu, Xu, lab_idx[:bt], unl_idx[:btu], cube, lab_pix, unl_pix)
        _chk_idx(lab_idx, "lab_idx")
        _chk_idx(unl_idx, "unl_idx")
        self._pl_truth = eng._pl_truth(unl_truth, Xu.shape[0]) if eng.pl_block is not None else None
        # the launchers set their kernels' LDS attributes on first use, which must not happen inside a capture
        if eng.step_count == 0:
            raise RuntimeError(f"run one eager {type(eng).__name__}.step() before capturing (kernel attributes are set lazily)")
        self._keep = (XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, cube, lab_pix, unl_pix)
        self.validate_indices()
        self.n_lab_idx, self.n_unl_idx = int(lab_idx.shape[0]), int(unl_idx.shape[0])
        # row 0 = the working copy the kernels read, rows 1 .. k the programmed steps, one spare row behind them
        self.table = torch.zeros((self.capacity + 2) * 64, dtype=torch.uint8, device=eng.device)
        self.cursor = torch.ones(1, dtype=torch.int32, device=eng.device)
        self.host = torch.zeros((self.capacity + 2) * 64, dtype=torch.uint8).pin_memory()
        self.rows = self.host.numpy().view(np.dtype(_lib.DYN_DTYPE))[1:]
        self.pending = self._programmed = 0
        self._copied = None       # event behind the last program()'s copy out of the pinned rows

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def validate_indices(self) -> None:
        """Range check of the two index buffers (synchronising): at capture, and whenever the caller has re-filled them
        in place and wants the check (the kernels follow the indices blindly)."""
        _, Xl, _, _, Xu, lab_idx, unl_idx = self._keep[:7]
        TrainEngine.check_index_range(lab_idx, Xl.shape[0], "lab_idx")
        TrainEngine.check_index_range(unl_idx, Xu.shape[0], "unl_idx")

    def program(self, steps) -> None:
        """``steps``: (epoch, batch_index, lab_off, unl_off) of the next replays, in order.  Fills the table from the
        engine's current state and rewinds the cursor (stream-ordered: behind every replay enqueued so far)."""
        eng, hp = self.eng, self.eng.hp
        steps = list(steps)
        if self.pending:
            raise RuntimeError(f"{self.pending} programmed steps have not been launched")
        if not 1 <= len(steps) <= self.capacity:
            raise ValueError(f"1..{self.capacity} steps per program")
        if self._copied is not None:
            self._copied.synchronize()        # the previous program's staging rows have left the pinned buffer
        k = len(steps)
        st = np.asarray(steps, dtype=np.int64).reshape(k, 4)
        if (st[:, 2:] < 0).any() or (st[:, 2] + self.bt > self.n_lab_idx).any() or (st[:, 3] + self.btu > self.n_unl_idx).any():
            raise ValueError("batch offsets outside the index buffers")
        rows = self.rows[:k]
        for name, col in replay_counters(eng.ptr, eng.adam_t, eng.step_count, eng.Q, hp.bank_step, eng.hist_rows,
                                         eng.method, k).items():
            rows[name] = col
        rows["lab_off"], rows["unl_off"] = st[:, 2], st[:, 3]
        rows["smooth"] = [1 if hp.smooth_gate(int(e), int(bi)) else 0 for e, bi in st[:, :2]]
        adap = {int(e): float(hp.thr * hp.adap_thr(int(e))) for e in np.unique(st[:, 0])}
        rows["adap_mask"] = [adap[int(e)] for e in st[:, 0]]
        a, b = C.c_float(), C.c_float()       # Adam's two scalars: formed by the library, exactly as the eager step does
        ss, bc = np.empty(k, np.float32), np.empty(k, np.float32)
        if eng.optim is None:
            for i in range(k):
                eng.lib.cmlpl_dyn_adam(C.byref(eng._chp), eng.adam_t + 1 + i, C.byref(a), C.byref(b))
                ss[i], bc[i] = a.value, b.value
        else:
            # the scheduled rate of each row goes through the same float32 as an eager step's hp copy; the decay factor
            # travels as its bit pattern in the row's `reserved`
            c, keep = C.c_float(), np.empty(k, np.float32)
            for i in range(k):
                t = eng.adam_t + 1 + i
                _lib.check("cmlpl_dyn_adam_opt", eng.lib.cmlpl_dyn_adam_opt(
                    C.byref(eng._hp_at(t)), t, float(eng.optim.weight_decay), C.byref(a), C.byref(b), C.byref(c)))
                ss[i], bc[i], keep[i] = a.value, b.value, c.value
            rows["reserved"] = keep.view(np.int32)
        rows["adam_step_size"], rows["adam_bc2_sqrt"] = ss, bc
        self.host[:64].copy_(self.host[64:128])            # row 0: the working copy starts as the first step's row
        k = (k + 1) * 64
        self.table[:k].copy_(self.host[:k], non_blocking=True)
        self.cursor.fill_(1)
        self.pending = self._programmed = len(steps)
        eng._graph = weakref.ref(self)
        # (the pinned staging rows may be rewritten only after that copy has run)
        self._copied = torch.cuda.Event()
        self._copied.record(torch.cuda.current_stream(eng.device))


class StepGraph(_ReplayTable):
    """The training step as a replayable hipGraph (SURVEY.md section 7 stage 6; ``cmlpl_step_graph_create``).

    Everything that changes from step to step -- random-stream counter, Adam step, bank pointers, the train.py:212 /
    :221 gates, the offsets of the batch inside the index buffers, the row of the logging ring -- lives in a device
    table of ``cmlpl_dyn`` rows that ``program()`` fills for a run of steps ahead of time (an epoch, say); a device
    cursor walks it, advanced by the step itself.  ``launch()`` is then ONE hipGraphLaunch per step: no arguments to
    marshal, nothing else enqueued.  The engine's host-side bookkeeping advances exactly as in ``TrainEngine.step``,
    so eager steps and replays can be mixed (an epoch's short last batch runs eagerly: its shape is not the graph's)
    -- but only BETWEEN programs: an eager step while programmed replays are pending raises (their rows were formed
    from the state before it).
    """

    def __init__(self, eng: TrainEngine, XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, bt: int, btu: int, capacity: int = 1024,
                 cube=None, lab_pix=None, unl_pix=None, unl_truth=None):
        super().__init__(eng, XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, bt, btu, capacity, cube, lab_pix, unl_pix, unl_truth)
        dev = eng.device
        eng._ensure_packed(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        io = _lib.StepIO()
        eng._fill_state(io)
        _fill_rows(io, XPl, Xl, Y, XPu, Xu, lab_idx, unl_idx, self.bt, self.btu, cube, lab_pix, unl_pix)
        io.d_scalars = eng.scalar_hist.data_ptr()          # ring base: the row comes from the table
        io.apply_update = 1
        io.d_dyn_table, io.d_dyn_cursor = self.table.data_ptr(), self.cursor.data_ptr()
        self._io = io
        eng._captured = True
        cap = torch.cuda.Stream(device=dev)
        cap.wait_stream(torch.cuda.current_stream(dev))
        handle = C.c_void_p()
        with torch.cuda.stream(cap):
            if eng.optim is None:
                _lib.check("cmlpl_step_graph_create", eng.lib.cmlpl_step_graph_create(
                    C.byref(eng.cshape), C.byref(eng._chp), C.byref(io), C.c_void_p(cap.cuda_stream), C.byref(handle)))
            else:        # the norms ring by its base, as the scalars' ring: the row comes from the table
                opt = eng._make_opt(eng.norm_hist.data_ptr())
                _lib.check("cmlpl_step_graph_create_opt", eng.lib.cmlpl_step_graph_create_opt(
                    C.byref(eng.cshape), C.byref(eng._chp), C.byref(io), C.byref(opt), C.c_void_p(cap.cuda_stream),
                    C.byref(handle)))
        torch.cuda.current_stream(dev).wait_stream(cap)
        self.handle = handle

    def launch(self) -> None:
        """one replay = one training step (asynchronous)"""
        eng = self.eng
        if self.pending < 1:
            raise RuntimeError("no programmed step left: call program() first")
        stream = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
        eng._ensure_packed(stream)            # set_params / load_state_dict between replays: the packed copies follow
        eng._teacher_begin()
        _lib.check("cmlpl_step_graph_launch", eng.lib.cmlpl_step_graph_launch(self.handle, stream))
        if eng.teacher is not None:           # one eager launch behind the replay: the captured step is what it was
            eng._teacher_update(stream)
        eng._advance(self.bt + self.btu, True)
        eng._last_btu = self.btu
        if eng.pl_block is not None:
            # one eager launch behind the replay: the threshold and the batch's place in the index buffer are those of
            # the programmed row this replay has just run (the float32 the step read, not a value formed anew)
            row = self.rows[self._programmed - self.pending]
            unl_idx = self._keep[6]
            eng._pl_update(stream, self._pl_truth, C.c_void_p(unl_idx.data_ptr() + 8 * int(row["unl_off"])), self.btu,
                           float(row["adap_mask"]))
        self.pending -= 1

    def close(self) -> None:
        if self.handle:
            self.eng.lib.cmlpl_step_graph_destroy(self.handle)
            self.handle = None
