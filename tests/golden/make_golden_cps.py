#!/usr/bin/env python3
"""Generate the cross-pseudo-supervision fixtures by running THE REFERENCE'S OWN STEP TEXT on CPU.

Run in the build container only (needs /root/reference):
    python tests/golden/make_golden_cps.py

On the pattern of make_golden.py (whose helpers it uses): ``trian_CPS.py`` cannot be imported (its line 11 imports a
module the reference does not ship), so it is read as text; lines 188-258 -- the inline step from ``Base.train()`` to
the last ``loss_hist`` column -- are dedented and exec'd in a namespace that supplies ``main()``'s locals: the
reference's own ``BaseNet2`` (loaded by file path), two ``torch.optim.Adam``, ``cls_loss``, ``args``, ``loss_hist``.
``.cuda()`` is the identity, ``torch.randn`` is served from the explicit draws of ``oracle.cmlpl_oracle.
synthetic_batch`` and dropout from its explicit masks.  The two ``zero_grad()`` calls of :185-186 lie in front of the
extract and are made here.

Pseudo-labels are an argmax: a row whose two largest logits sit within rounding of each other could flip between two
hosts.  CONDITION (asserted here on the reference's own logits, stored in the file, re-asserted by the GPU test): every
unlabelled row of every step has top-1 minus top-2 logit >= 1e-3 in BOTH networks; no row is left out.  The seed walks
upward from 0 until a case satisfies it.

Only inputs-by-seed and OUTPUT ARRAYS are stored (tests/golden/cps/cps_*.npz); no reference source.
"""
import os
import sys
import textwrap
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tests.golden import make_golden as MG  # noqa: E402  (build_ref_net, TorchProxy, MaskDrop; patches .cuda())
from oracle import cmlpl_oracle as O  # noqa: E402  (input generators only)

OUT = os.path.join(HERE, "cps")
MARGIN_MIN = 1e-3
LIVE = O.LIVE_KEYS
FULL_PARAMS = ("conv0.bias", "conv1.bias", "conv2.bias", "classifier.bias")      # small tensors stored whole after Adam

with open(os.path.join(MG.REF, "trian_CPS.py")) as fh:
    _lines = fh.read().split("\n")
STEP_SRC = textwrap.dedent("\n".join(_lines[187:258]))      # trian_CPS.py:188-258
STEP_CODE = compile(STEP_SRC, "<reference trian_CPS.py:188-258>", "exec")


def margin(z):
    t = torch.topk(z.detach(), 2, dim=1)[0]
    return float((t[:, 0] - t[:, 1]).min())


def try_case(shape, bt, btu, steps, seed, dropout, separable):
    """the case at one seed: its arrays, or None when a row misses the margin condition"""
    hp = O.HyperParams(dropout=dropout)
    args = types.SimpleNamespace(noise=hp.noise, lr=hp.lr)
    Base = MG.build_ref_net(shape, O.closed_form_params(shape, seed), dropout)
    Base1 = MG.build_ref_net(shape, O.closed_form_params(shape, seed + 1), dropout)
    tp = MG.TorchProxy()
    ns = dict(args=args, Base=Base, Base1=Base1, cls_loss=torch.nn.CrossEntropyLoss(),
              base_optimizer=torch.optim.Adam(Base.parameters(), lr=args.lr),
              base1_optimizer=torch.optim.Adam(Base1.parameters(), lr=args.lr),
              loss_hist=np.zeros((steps, 5)), index_i=-1, torch=tp, np=np)
    rec = {k: [] for k in ("hist", "extra", "pseudo", "agree", "margins", "logits", "grad_norms", "param_sums",
                           "grad_cls", "params_after")}
    for s in range(steps):
        b = O.synthetic_batch(shape, bt, btu, seed * 1000 + s, dropout=dropout, separable=separable)
        tp.queue = list(b["noise"])
        Base.drop.mask, Base1.drop.mask = b["dropmask"]
        ns["index_i"] += 1                                                        # :183
        ns["base1_optimizer"].zero_grad()                                         # :185
        ns["base_optimizer"].zero_grad()                                          # :186
        ns.update(labeled_data=(b["XPl"], b["Xl"], b["Y"]),
                  unlabeled_data=(b["XPu"], b["Xu"], torch.zeros(btu, dtype=torch.long)))
        exec(STEP_CODE, ns)
        assert not tp.queue
        m = [margin(ns["un_b_output"]), margin(ns["un_e_output"])]
        if min(m) < MARGIN_MIN:
            return None
        rec["margins"].append(m)
        rec["hist"].append(ns["loss_hist"][ns["index_i"]].copy())
        rec["extra"].append([ns["total_loss1"].item(), ns["cls_loss_value1"].item(), ns["con_loss_value1"].item()])
        # [0] = what Base learns from (Base1's argmax, :239), [1] = what Base1 learns from (Base's argmax, :238)
        rec["pseudo"].append(np.stack([ns["UNlabeled_prd2"].numpy(), ns["UNlabeled_prd1"].numpy()]))
        rec["agree"].append(int((ns["UNlabeled_prd1"] == ns["UNlabeled_prd2"]).sum()))
        rec["logits"].append(np.stack([ns["un_b_output_all"].detach().numpy(), ns["un_e_output_all"].detach().numpy()]))
        gn, psum, gc, pa = [], [], [], []
        for net in (Base, Base1):
            sd = dict(net.named_parameters())
            gn.append([sd[k].grad.double().norm().item() for k in LIVE])
            psum.append([sd[k].detach().double().sum().item() for k in LIVE])
            gc.append(sd["classifier.weight"].grad.numpy()[:, :16].copy())
            pa.append(np.concatenate([sd[k].detach().numpy().reshape(-1) for k in FULL_PARAMS]))
            for k, prm in net.named_parameters():
                if k not in LIVE:
                    assert prm.grad is None        # dead parameters
        rec["grad_norms"].append(gn); rec["param_sums"].append(psum); rec["grad_cls"].append(gc)
        rec["params_after"].append(pa)
    return rec


def run_case(name, shape, bt, btu, steps, dropout=0.8, separable=0.0, max_seed=400):
    for seed in range(max_seed):
        rec = try_case(shape, bt, btu, steps, seed, dropout, separable)
        if rec is not None:
            break
    else:
        raise SystemExit(f"{name}: no seed below {max_seed} meets the margin condition (raise separable)")
    mmin = float(np.min(rec["margins"]))
    assert mmin >= MARGIN_MIN
    out = dict(hist=np.asarray(rec["hist"], np.float64), extra=np.asarray(rec["extra"], np.float64),
               pseudo=np.asarray(rec["pseudo"], np.int64), agree=np.asarray(rec["agree"], np.int64),
               margins=np.asarray(rec["margins"], np.float64), logits=np.asarray(rec["logits"], np.float32),
               grad_norms=np.asarray(rec["grad_norms"], np.float64), param_sums=np.asarray(rec["param_sums"], np.float64),
               grad_cls=np.asarray(rec["grad_cls"], np.float32), params_after=np.asarray(rec["params_after"], np.float32),
               cfg=np.asarray([shape.C, shape.H, shape.W, shape.bands, shape.K, bt, btu, steps, seed], np.int64),
               cfg_f=np.asarray([dropout, separable, mmin], np.float64))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: seed {seed}, {steps} steps, smallest margin {mmin:.3e}, last hist={rec['hist'][-1]}, "
          f"agree={rec['agree']}, {os.path.getsize(path) / 1024:.1f} KB")


def main():
    P = O.NetShape(60, 20, 20, 103, 9)          # the only shape the reference constructs
    B2 = O.NetShape(103, 11, 11, 103, 9)
    B5 = O.NetShape(48, 15, 15, 48, 16)         # Houston-shaped window, K = 16 (a full power-of-two class count)
    run_case("cps_b2_32x3", B2, 32, 32, steps=3)           # Adam moments carry over three consecutive steps
    run_case("cps_p_16", P, 16, 16, steps=1)               # the reference's own shape
    run_case("cps_b5_8to64", B5, 8, 64, steps=1)           # bt != btu, K = 16


if __name__ == "__main__":
    main()
