"""CPU restatement of one cross-pseudo-supervision training step (reference trian_CPS.py:188-258), built from the
oracle's pieces (oracle/cmlpl_oracle.py: ``basenet2_forward``, ``adam_update``, ``StepState``).  TEST INFRASTRUCTURE.

Pinned by tests/test_cps_golden.py against fixtures the reference's own step text produced
(tests/golden/make_golden_cps.py); from there on it is the yardstick for shapes the fixtures do not cover.

Reference lines restated (all trian_CPS.py):
  * input augmentation ............ :191-192,198-199,209-210,221-222 (the draw order of train.py's step)
  * the two forwards .............. :211-213, :223-225
  * supervised CE / accuracy ...... :234-237, :258
  * hard pseudo-labels ............ :238-239 (torch.max: first maximum)
  * cross losses .................. :241-244
  * totals / backward / Adam ...... :245-250 (weight 0.1)
  * logged row .................... :254-258 (column 0 repeats the cross loss)
"""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cmlpl_oracle as O

CPS_W = 0.1                                                                  # literal of :245,248
CPS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cps")
MARGIN_MIN = 1e-3      # every unlabelled row of every fixture: top-1 minus top-2 logit, ten times the 1e-4 logits are compared at


def cps_loss_block(z_s, z_w, Y, bt, w=CPS_W):
    """z_*: logits [n][K] of Base (s) / Base1 (w), rows [:bt] labelled.  Autograd-connected totals + every intermediate."""
    zL_s, zU_s, zL_w, zU_w = z_s[:bt], z_s[bt:], z_w[:bt], z_w[bt:]
    cls_s = F.cross_entropy(zL_s, Y)                                         # :234
    cls_w = F.cross_entropy(zL_w, Y)                                         # :235
    acc = (torch.max(zL_w, 1)[1] == Y).float().mean()                        # :237,258
    t_w = torch.max(zU_s.detach(), 1)[1]                                     # :238  UNlabeled_prd1 (Base's argmax)
    t_s = torch.max(zU_w.detach(), 1)[1]                                     # :239  UNlabeled_prd2 (Base1's argmax)
    con_s = F.cross_entropy(zU_s, t_s)                                       # :241,243
    con_w = F.cross_entropy(zU_w, t_w)                                       # :242,244
    return dict(total_s=cls_s + w * con_s, total_w=cls_w + w * con_w,        # :245,248
                cls_s=cls_s, cls_w=cls_w, con_s=con_s, con_w=con_w, acc=acc,
                pseudo=torch.stack([t_s, t_w]), agree=int((t_s == t_w).sum()))


def top2_margin(z):
    """smallest (top-1 minus top-2) over the rows of z [rows][K]"""
    t = torch.topk(z.detach(), 2, dim=1)[0]
    return float((t[:, 0] - t[:, 1]).min())


def cps_step(state, batch, hp=None, apply_update=True, relu_gates=None, w=CPS_W):
    """One CPS step on ``batch`` (``O.synthetic_batch``'s dict: XPl, Xl, Y, XPu, Xu, the 8 noise draws in the
    reference's order, 2 dropout masks).  Mutates ``state`` (parameters, Adam moments); its banks and pointers are not
    touched.  ``relu_gates``: the device's activation patterns (tests/gpu_util.py)."""
    hp = hp or O.HyperParams()
    XPl, Xl, Y, XPu, Xu, noise, dropmask = (batch[k] for k in ("XPl", "Xl", "Y", "XPu", "Xu", "noise", "dropmask"))
    bt, sg = XPl.shape[0], hp.noise
    XP_b_all = torch.cat([XPl + noise[0] * sg, XPu + noise[4] * sg], 0)      # :191,209,211
    X_b_all = torch.cat([Xl + noise[1] * sg, Xu + noise[5] * sg], 0)         # :192,210,212
    XP_e_all = torch.cat([XPl + noise[2] * sg, XPu + noise[6] * sg], 0)      # :198,221,223
    X_e_all = torch.cat([Xl + noise[3] * sg, Xu + noise[7] * sg], 0)         # :199,222,224
    ps = [{k: (v.detach().clone().requires_grad_(True) if k in O.LIVE_KEYS else v) for k, v in state.params[net].items()}
          for net in range(2)]
    taps = [{}, {}]
    rg = relu_gates or (None, None)
    z_s, f_s = O.basenet2_forward(ps[0], XP_b_all, X_b_all, dropmask[0], taps[0], rg[0])   # :213
    z_w, f_w = O.basenet2_forward(ps[1], XP_e_all, X_e_all, dropmask[1], taps[1], rg[1])   # :225
    lb = cps_loss_block(z_s, z_w, Y, bt, w)
    g_s = torch.autograd.grad(lb["total_s"], [ps[0][k] for k in O.LIVE_KEYS])               # :246
    g_w = torch.autograd.grad(lb["total_w"], [ps[1][k] for k in O.LIVE_KEYS])               # :249
    grads = [dict(zip(O.LIVE_KEYS, g_s)), dict(zip(O.LIVE_KEYS, g_w))]
    if apply_update:
        for net in range(2):                                                                # :247,250
            st = state.adam[net]
            st.t += 1
            for k in O.LIVE_KEYS:
                O.adam_update(state.params[net][k], grads[net][k], st.m[k], st.v[k], st.t, hp)
    out = dict(lb)
    out.update(logits=[z_s.detach(), z_w.detach()], feats=[f_s.detach(), f_w.detach()], grads=grads, taps=taps,
               margin=min(top2_margin(z_s[bt:]), top2_margin(z_w[bt:])),
               hist=[float(lb[k].detach()) for k in ("con_s", "total_s", "cls_s", "con_s", "acc")],      # :254-258
               extra=[float(lb[k].detach()) for k in ("total_w", "cls_w", "con_w")])
    return out


def cps_cases():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(CPS_DIR, "cps_*.npz")))


class CpsCase:
    """a fixture of tests/golden/make_golden_cps.py"""

    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(CPS_DIR, name + ".npz"))
        c = self.z["cfg"]
        self.shape = O.NetShape(int(c[0]), int(c[1]), int(c[2]), int(c[3]), int(c[4]))
        self.bt, self.btu, self.steps, self.seed = int(c[5]), int(c[6]), int(c[7]), int(c[8])
        self.dropout, self.separable, self.margin = (float(v) for v in self.z["cfg_f"])
        self.hp = O.HyperParams(dropout=self.dropout)

    def params(self):
        return O.closed_form_params(self.shape, self.seed), O.closed_form_params(self.shape, self.seed + 1)

    def batch(self, s):
        return O.synthetic_batch(self.shape, self.bt, self.btu, self.seed * 1000 + s, dropout=self.dropout,
                                 separable=self.separable)
