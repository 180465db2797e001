"""CPU: the contract of the C entry points that no launch count can see -- the workspace layout and the precedence of
the return codes -- held to a record of what the library answered BEFORE the entry points were reorganised around one
step context (api.hip / api_infer.hip / api_aux.hip).

tests/golden/api_contract.json was generated from the PARENT commit's library, not from this tree: default switches, no
device (the library then plans for 256 compute units).  To regenerate it, build the commit whose behaviour is the
reference and run this module as a script with CMLPL_LIB naming that build:

    CMLPL_LIB=/path/to/reference/libcmlpl_hip.so python -m tests.test_api_contract_cpu

Part 1 (sizes): for every (shape, n) of tests/envelope_cases.CASES, the four bench.py workloads at n = 256, and one or
two networks -- cmlpl_workspace_bytes, every region cmlpl_debug_region names, the loss and inference workspaces, the route
and the 3x3 weight-gradient plan.  Equal integer for integer.

Part 2 (refusals): malformed calls with fake non-null pointers.  Every row is refused by the argument checks, which run
in front of any device call, so the pointers are never followed; a call that would pass them is never made (the recorder
rejects a row whose reference answer is not a negative CMLPL_E_* code).  Rows with two faults at once pin which check
comes first."""
import ctypes as C
import json
import os

import pytest

from tests.envelope_cases import CASES

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_contract.json")
FAKE = 0x10000          # a non-null "device pointer", 16-byte aligned, never dereferenced
BIG = 1 << 40
GOOD, BAD, NOROUTE = (103, 11, 11, 103, 9), (103, 11, 11, 103, 65), (3, 24, 24, 5, 3)   # K > 64; in range but no route takes it
BENCH = {"B2": (103, 11, 11, 103, 9), "P": (60, 20, 20, 103, 9), "B4": (200, 11, 11, 200, 16), "B5": (48, 15, 15, 48, 20)}
REGIONS = ("a0", "p1", "m1", "p2", "m2", "y", "ynorm", "catd", "dropgen", "dy", "dp2", "dp1", "da0", "xn", "probs",
           "cps_pseudo")
HP = (5e-4, 0.9, 0.999, 1e-8, 0.3, 0.95, 0.5, 0.8, 0.5, 4.0, 0.8, 0.3)      # _lib.HParams in field order
BT = BTU = 8
N = BT + BTU


def up256(v):
    return (v + 255) & ~255


# ---------------------------------------------------------------------------------------------------- part 1: sizes
def size_cases():
    seen = [(c.shape, c.n) for c in CASES] + [(s, 256) for s in BENCH.values()]
    return [(s, n, nets) for s, n in dict.fromkeys(seen) for nets in (1, 2)]


def size_key(shape, n, nets):
    return "x".join(map(str, shape)) + f"-n{n}-nets{nets}"


def sizes_of(lib, shape, n, nets):
    from cmlpl_amd import _lib
    cs = _lib.Shape(*shape)
    sp = C.byref(cs)
    rec = {"workspace": [lib.cmlpl_workspace_bytes(sp, nets, n, n), lib.cmlpl_workspace_bytes(sp, nets, n, 10 * n)]}
    rec["regions"] = {}
    for name in REGIONS:
        off, size = C.c_size_t(0), C.c_size_t(0)
        rc = lib.cmlpl_debug_region(sp, nets, n, name.encode(), C.byref(off), C.byref(size))
        rec["regions"][name] = [off.value, size.value] if rc == 0 else rc
    bt, btu = n // 2, n - n // 2
    one, two = _lib.Shard(bt, btu, 0, bt, 0, btu), _lib.Shard(2 * bt, 2 * btu, bt, bt, btu, btu)
    rec["loss_workspace"] = [lib.cmlpl_loss_workspace_bytes(sp, C.byref(one), 10 * n),
                             lib.cmlpl_loss_workspace_bytes(sp, C.byref(two), 20 * n)]
    rec["infer_workspace"] = [lib.cmlpl_infer_workspace_bytes(C.addressof(cs), n), lib.cmlpl_eval_workspace_bytes(sp, nets, n),
                              lib.cmlpl_infer_tta_workspace_bytes(sp, n), lib.cmlpl_eval_tta_workspace_bytes(sp, nets, n)]
    route, plan = (C.c_int * 30)(), (C.c_int * 17)()
    rec["route"] = [lib.cmlpl_debug_route(sp, nets, n, route)] + list(route)
    rec["wgrad3_plan"] = [lib.cmlpl_debug_wgrad3_plan(sp, nets, n, plan)] + list(plan)
    return rec


# ------------------------------------------------------------------------------------------------ part 2: refusals
# An entry point's arguments in the header's order, each with the value of a WELL-FORMED call; a row overrides some.
# Records (hp, batch, shard, banks, gathered, opt, io, dio) are given as a dict of field overrides, or None for a null.
PTR = dict(params=FAKE, packed=FAKE, dropmask=None, stream=None, ws=FAKE, ws_bytes="big")
NET = dict(shape=GOOD, nets=2, n=N, pstride=0, dropout=0.3, train=1, seed=1, step=0, shard=None)
PASS = dict(shape=GOOD, hp={}, batch={}, shard=None, train=1, seed=1, step=0)
LOSS = dict(shape=GOOD, shard={}, logits=FAKE, feat=FAKE, labels=FAKE, banks={}, smooth=1, adap=0.5, hp={}, gathered={},
            probs_g=FAKE, pshard=BTU, scalars=FAKE, dlogits=FAKE, dfeat=FAKE, probs=FAKE, dfw=FAKE, ws=FAKE, ws_bytes="big",
            stream=None, bt=BT, btu=BTU)
ENTRY = {
    "cmlpl_basenet2_fwd": (dict(NET, **PTR, xn=FAKE, sn=FAKE, snT=None, logits=FAKE, feat=FAKE),
                           "shape nets n params pstride packed xn sn snT dropmask dropout train seed step shard logits feat "
                           "ws ws_bytes stream"),
    "cmlpl_basenet2_bwd": (dict(NET, **PTR, xn=FAKE, sn=FAKE, dlogits=FAKE, dfeat=FAKE, grads=FAKE, gstride=0),
                           "shape nets n params pstride packed xn sn dropmask dropout train dlogits dfeat grads gstride ws "
                           "ws_bytes stream"),
    "cmlpl_forward": (dict(PASS, **PTR, logits=FAKE, feat=FAKE, labels_f=None),
                      "shape hp batch shard params packed dropmask train seed step logits feat labels_f ws ws_bytes stream"),
    "cmlpl_forward_spectral": (dict(PASS, **PTR, feat=FAKE, labels_f=None),
                               "shape hp batch shard params seed step feat labels_f ws ws_bytes stream"),
    "cmlpl_forward_spatial": (dict(PASS, **PTR, logits=FAKE),
                              "shape hp batch shard params packed dropmask train seed step logits ws ws_bytes stream"),
    "cmlpl_backward": (dict(PASS, **PTR, dlogits=FAKE, dfeat=FAKE, grads=FAKE, gstride=0),
                       "shape hp batch shard params packed dropmask train seed step dlogits dfeat grads gstride ws ws_bytes "
                       "stream"),
    "cmlpl_backward_data": (dict(PASS, **PTR, dlogits=FAKE),
                            "shape hp batch shard params packed dropmask train seed step dlogits ws ws_bytes stream"),
    "cmlpl_backward_weights": (dict(PASS, **PTR, dlogits=FAKE, dfeat=FAKE, grads=FAKE, gstride=0),
                               "shape hp batch shard params packed dropmask train seed step dlogits dfeat grads gstride ws "
                               "ws_bytes stream"),
    "cmlpl_loss_phase1": (LOSS, "shape shard logits feat labels banks smooth adap hp dlogits dfeat probs ws ws_bytes stream"),
    "cmlpl_loss_phase2": (LOSS, "shape shard logits feat labels banks smooth adap hp probs_g pshard scalars dfeat dfw ws "
                                "ws_bytes stream"),
    "cmlpl_loss_phase1_g": (LOSS, "shape shard gathered banks smooth adap hp dlogits dfeat probs ws ws_bytes stream"),
    "cmlpl_loss_phase2_g": (LOSS, "shape shard gathered banks smooth adap hp probs_g pshard scalars dfeat dfw ws ws_bytes "
                                  "stream"),
    "cmlpl_loss_fwd_bwd": (LOSS, "shape bt btu logits feat labels banks smooth adap hp scalars dlogits dfeat probs ws "
                                 "ws_bytes stream"),
    "cmlpl_cps_loss_fwd_bwd": (dict(LOSS, pseudo=FAKE), "shape bt btu logits labels hp scalars dlogits pseudo ws ws_bytes "
                                                        "stream"),
    "cmlpl_adam_step_opt": (dict(shape=GOOD, nets=2, params=FAKE, pstride=BIG, grads=FAKE, gstride=BIG, m=FAKE, v=FAKE, t=1,
                                 hp={}, packed=FAKE, opt={}, stream=None),
                            "shape nets params pstride grads gstride m v t hp packed opt stream"),
    "cmlpl_grad_norm": (dict(shape=GOOD, nets=2, grads=FAKE, gstride=BIG, max_norm=1.0, partials=FAKE, norms=FAKE,
                             stream=None), "shape nets grads gstride max_norm partials norms stream"),
    "cmlpl_train_step": (dict(shape=GOOD, hp={}, io={}, stream=None), "shape hp io stream"),
    "cmlpl_train_step_opt": (dict(shape=GOOD, hp={}, io={}, opt={}, stream=None), "shape hp io opt stream"),
    "cmlpl_step_graph_create": (dict(shape=GOOD, hp={}, io={}, stream=None, graph_out=True), "shape hp io stream graph_out"),
    "cmlpl_step_graph_create_opt": (dict(shape=GOOD, hp={}, io={}, opt={}, stream=None, graph_out=True),
                                    "shape hp io opt stream graph_out"),
    "cmlpl_dist_stage_graph_create": (dict(shape=GOOD, hp={}, dio={}, stage=0, stream=None, graph_out=True),
                                      "shape hp dio stage stream graph_out"),
    "cmlpl_debug_region": (dict(shape=GOOD, nets=2, n=N, name=b"a0", off=True, size=True), "shape nets n name off size"),
}


def _merge(defaults, over):
    out = dict(defaults)
    for k, v in over.items():
        out[k] = _merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def _fill(rec, defaults, over):
    for k, v in _merge(defaults, over).items():
        if isinstance(v, dict):
            _fill(getattr(rec, k), {}, v)
        elif isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                getattr(rec, k)[i] = x
        else:
            setattr(rec, k, v)
    return rec


def _records(lib):
    """field defaults of the well-formed records"""
    from cmlpl_amd import _lib
    banks = dict(d_feats=(FAKE, FAKE), d_probs=(FAKE, FAKE), Q=10 * N)
    batch = dict(d_xpl=FAKE, d_xl=FAKE, d_xpu=FAKE, d_xu=FAKE, d_labels=FAKE, bt=BT, btu=BTU)
    shard = dict(bt_g=BT, btu_g=BTU, lab0=0, nlab=BT, unl0=0, nunl=BTU)
    io = dict(batch, banks=banks, workspace_bytes=BIG, adam_t=1, apply_update=1,
              **{k: FAKE for k in ("d_params", "d_m", "d_v", "d_grads", "d_packed", "d_scalars", "d_logits", "d_feat",
                                   "d_workspace")})
    dio = dict(batch=dict(batch, d_lab_idx=FAKE, d_unl_idx=FAKE), shard=shard, banks=banks, d_dyn_table=FAKE,
               d_dyn_cursor=FAKE)
    return {"hp": (_lib.HParams, dict(zip((f[0] for f in _lib.HParams._fields_), HP))), "batch": (_lib.Batch, batch),
            "shard": (_lib.Shard, shard), "banks": (_lib.Banks, banks), "io": (_lib.StepIO, io), "dio": (_lib.DistIO, dio),
            "gathered": (_lib.Gathered, dict(d_recv_feat=FAKE, d_logits_local=FAKE, world=1, bt_local=BT, btu_local=BTU)),
            "opt": (_lib.Optim, dict(max_norm=0.0, weight_decay=0.0, d_norms=None, d_partials=None))}


def _bytes_needed(lib, what, shape):
    """workspace sizes of the well-formed calls, from the library itself; `what` - 1 is one byte short"""
    from cmlpl_amd import _lib
    cs = _lib.Shape(*shape)
    sp = C.byref(cs)
    off, size = C.c_size_t(0), C.c_size_t(0)
    assert lib.cmlpl_debug_region(sp, 2, N, b"xn", C.byref(off), C.byref(size)) == 0
    if what == "net":           # the two networks' regions
        return off.value
    if what == "pass":          # ... and the step's rows: what a forward or backward alone needs
        return off.value + up256(size.value) + up256(2 * N * shape[3] * 4)
    if what == "step":          # everything (cmlpl_workspace_bytes adds 256 for the caller's alignment)
        return lib.cmlpl_workspace_bytes(sp, 2, N, 10 * N) - 256
    if what == "loss":
        sh = _lib.Shard(BT, BTU, 0, BT, 0, BTU)
        return lib.cmlpl_loss_workspace_bytes(sp, C.byref(sh), 10 * N)
    assert what == "cps"
    return lib.cmlpl_cps_loss_workspace_bytes(sp, BT, BTU)


def call(lib, fn, over):
    from cmlpl_amd import _lib
    defaults, order = ENTRY[fn]
    recs, keep, args = _records(lib), [], []
    v = dict(defaults, **over)
    shape = v["shape"] or GOOD
    for name in order.split():
        x = v[name]
        if name == "shape":
            x = _lib.Shape(*x) if x is not None else None
        elif name in recs and x is not None:
            x = _fill(recs[name][0](), recs[name][1], x)
            if name == "io" and "io_ws" in over:        # one byte short of what `io_ws` names
                x.workspace_bytes = _bytes_needed(lib, over["io_ws"], shape) - 1
        elif name in ("graph_out", "off", "size"):
            x = (C.c_void_p if name == "graph_out" else C.c_size_t)() if x else None
        elif name == "ws_bytes" and isinstance(x, str):
            x = BIG if x == "big" else _bytes_needed(lib, x.split("-")[0], shape) - 1
        if isinstance(x, (C.Structure, C._SimpleCData)):
            keep.append(x)
            x = C.byref(x)
        args.append(x)
    return getattr(lib, fn)(*args)


def _rows():
    rows = []

    def add(fn, tag, **over):
        rows.append((f"{fn[6:]}:{tag}", fn, over))

    def nulls(fn, names):
        for nm in names:
            add(fn, f"null-{nm}", **{nm: None})

    two = dict(shape=BAD)           # two faults: the shape is looked at first
    for fn in ("cmlpl_basenet2_fwd", "cmlpl_basenet2_bwd"):
        fwd = fn.endswith("fwd")
        nulls(fn, ("shape", "params", "packed", "xn", "sn", "ws") + (("logits", "feat") if fwd else ("dlogits", "grads")))
        add(fn, "bad-shape", shape=BAD); add(fn, "no-route", shape=NOROUTE)
        add(fn, "nets-0", nets=0); add(fn, "nets-3", nets=3); add(fn, "n-0", n=0)
        add(fn, "ws-short", ws_bytes="net-1")
        add(fn, "bad-shape+null", params=None, **two)
        add(fn, "no-route+null", shape=NOROUTE, params=None)
        add(fn, "null+ws-short", packed=None, ws_bytes="net-1")
        add(fn, "n-0+ws-short", n=0, ws_bytes=0)
        if fwd:
            add(fn, "dropout-1", dropout=1.0); add(fn, "dropout-neg", dropout=-0.25)
            add(fn, "dropout-1+ws-short", dropout=1.0, ws_bytes="net-1")
    for fn in ("cmlpl_forward", "cmlpl_forward_spectral", "cmlpl_forward_spatial", "cmlpl_backward", "cmlpl_backward_data",
               "cmlpl_backward_weights"):
        names = ENTRY[fn][1].split()
        req = {"cmlpl_forward": ("packed", "logits", "feat"), "cmlpl_forward_spectral": ("feat",),
               "cmlpl_forward_spatial": ("packed", "logits"), "cmlpl_backward": ("packed", "dlogits", "grads"),
               "cmlpl_backward_data": ("packed", "dlogits"), "cmlpl_backward_weights": ("packed", "dlogits", "grads")}[fn]
        nulls(fn, ("shape", "hp", "batch", "params", "ws") + req)
        add(fn, "bad-shape", shape=BAD); add(fn, "no-route", shape=NOROUTE)
        add(fn, "bt-0", batch=dict(bt=0)); add(fn, "btu-0", batch=dict(btu=0)); add(fn, "bt-neg", batch=dict(bt=-3))
        for f in ("d_xl", "d_xu", "d_xpl", "d_xpu"):
            add(fn, f"batch-null-{f}", batch={f: None})
        add(fn, "cube-with-rows", batch=dict(d_cube=FAKE, cube_rows=32, cube_cols=32, d_lab_pix=FAKE, d_unl_pix=FAKE))
        add(fn, "cube-too-small", batch=dict(d_xpl=None, d_xpu=None, d_cube=FAKE, cube_rows=5, cube_cols=32, d_lab_pix=FAKE,
                                             d_unl_pix=FAKE))
        add(fn, "ws-short", ws_bytes="pass-1")
        add(fn, "bad-shape+null", params=None, **two)
        add(fn, "no-route+null", shape=NOROUTE, params=None)
        add(fn, "null+ws-short", params=None, ws_bytes="pass-1")
        add(fn, "bad-batch+ws-short", batch=dict(d_xl=None), ws_bytes="pass-1")
        add(fn, "bt-0+ws-short", batch=dict(bt=0), ws_bytes=0)
        add(fn, "cube-too-small+null", batch=dict(d_xpl=None, d_xpu=None, d_cube=FAKE, cube_rows=5, cube_cols=32,
                                                  d_lab_pix=FAKE, d_unl_pix=FAKE), params=None)
        if "forward" in fn:
            add(fn, "dropout-1", hp=dict(dropout_p=1.0)); add(fn, "dropout-neg", hp=dict(dropout_p=-0.25))
            add(fn, "shard-mismatch", shard=dict(nlab=BT - 1))
            add(fn, "shard-mismatch-unl", shard=dict(nunl=BTU + 1))
            add(fn, "dropout-1+ws-short", hp=dict(dropout_p=1.0), ws_bytes="pass-1")
            add(fn, "shard-mismatch+no-route", shape=NOROUTE, shard=dict(nlab=BT - 1))
            if "labels_f" in names:
                add(fn, "labels_f-without-labels", labels_f=FAKE, batch=dict(d_labels=None))
    for fn in ("cmlpl_loss_phase1", "cmlpl_loss_phase2", "cmlpl_loss_phase1_g", "cmlpl_loss_phase2_g"):
        g, p2 = fn.endswith("_g"), "phase2" in fn
        outs = ("probs_g", "scalars", "dfeat", "dfw") if p2 else ("dlogits", "dfeat", "probs")
        nulls(fn, ("shape", "shard", "banks", "hp", "ws") + (("gathered",) if g else ("logits", "feat", "labels")) + outs)
        add(fn, "bad-shape", shape=BAD)
        add(fn, "shard-past-batch", shard=dict(lab0=1)); add(fn, "shard-no-unl", shard=dict(nunl=0))
        add(fn, "shard-btu-2049", shard=dict(btu_g=2049, nunl=BTU))
        add(fn, "banks-short", banks=dict(Q=N - 1)); add(fn, "banks-null", banks=dict(d_probs=(FAKE, None)))
        add(fn, "ws-short", ws_bytes="loss-1")
        add(fn, "bad-shape+null", hp=None, **two)
        add(fn, "null-in+ws-short", banks=None, ws_bytes="loss-1")
        add(fn, "null-out+ws-short", **{outs[0]: None}, ws_bytes="loss-1")      # the outputs are looked at last
        add(fn, "bad-shard+ws-short", shard=dict(nunl=0), ws_bytes="loss-1")
        if g:
            add(fn, "gathered-world", gathered=dict(world=2)); add(fn, "gathered-null-feat", gathered=dict(d_recv_feat=None))
            add(fn, "gathered-rows", gathered=dict(btu_local=BTU // 2))
            add(fn, "gathered-null+bad-shape", gathered=None, **two)
        if p2:
            add(fn, "pshard-0", pshard=0); add(fn, "pshard-odd", pshard=BTU - 1)
            add(fn, "pshard-odd+ws-short", pshard=BTU - 1, ws_bytes="loss-1")
    fn = "cmlpl_loss_fwd_bwd"
    nulls(fn, ("shape", "logits", "feat", "labels", "banks", "hp", "scalars", "dlogits", "dfeat", "probs", "ws"))
    add(fn, "bad-shape", shape=BAD); add(fn, "bt-0", bt=0); add(fn, "btu-0", btu=0); add(fn, "btu-2049", btu=2049)
    add(fn, "banks-short", banks=dict(Q=N - 1)); add(fn, "ws-short", ws_bytes="loss-1")
    add(fn, "bad-shape+null", probs=None, **two)
    add(fn, "null-out+ws-short", probs=None, ws_bytes="loss-1")                 # here the outputs are looked at first
    add(fn, "null-in+ws-short", feat=None, ws_bytes="loss-1"); add(fn, "bt-0+ws-short", bt=0, ws_bytes=0)
    fn = "cmlpl_cps_loss_fwd_bwd"
    nulls(fn, ("shape", "logits", "labels", "hp", "scalars", "dlogits", "pseudo", "ws"))
    add(fn, "bad-shape", shape=BAD); add(fn, "bt-0", bt=0); add(fn, "btu-0", btu=0); add(fn, "ws-short", ws_bytes="cps-1")
    add(fn, "bad-shape+null", hp=None, **two); add(fn, "null+ws-short", pseudo=None, ws_bytes="cps-1")
    add(fn, "bt-0+ws-short", bt=0, ws_bytes=0)
    nan, wanted = float("nan"), dict(max_norm=1.0, d_partials=FAKE)
    bad_opts = dict([("max_norm-neg", dict(max_norm=-1.0)), ("max_norm-nan", dict(max_norm=nan)),
                     ("max_norm-inf", dict(max_norm=float("inf"))), ("decay-neg", dict(weight_decay=-0.5)),
                     ("decay-nan", dict(weight_decay=nan)), ("norms-misaligned", dict(wanted, d_norms=FAKE + 2)),
                     ("partials-misaligned", dict(max_norm=1.0, d_partials=FAKE + 4)),
                     ("clip-without-partials", dict(max_norm=1.0)), ("norms-without-partials", dict(d_norms=FAKE))])
    kills = dict(hp=dict(lr=0.5), opt=dict(weight_decay=2.0))                   # 1 - lr * decay == 0
    fn = "cmlpl_adam_step_opt"
    add(fn, "opt-decay-kills-weights", **kills)
    nulls(fn, ("shape", "params", "grads", "m", "v", "hp"))
    add(fn, "bad-shape", shape=BAD); add(fn, "nets-0", nets=0); add(fn, "nets-3", nets=3); add(fn, "t-0", t=0)
    for tag, o in bad_opts.items():
        add(fn, "opt-" + tag, opt=o)
    add(fn, "opt-grad-stride-short", opt=wanted, gstride=16)
    add(fn, "bad-shape+null", m=None, **two); add(fn, "bad-shape+bad-opt", opt=dict(max_norm=-1.0), **two)
    add(fn, "null+bad-opt", v=None, opt=dict(max_norm=-1.0))
    fn = "cmlpl_grad_norm"
    nulls(fn, ("shape", "grads", "partials", "norms"))
    add(fn, "bad-shape", shape=BAD); add(fn, "nets-0", nets=0); add(fn, "nets-3", nets=3); add(fn, "stride-short", gstride=16)
    add(fn, "max_norm-neg", max_norm=-1.0); add(fn, "max_norm-nan", max_norm=nan)
    add(fn, "partials-misaligned", partials=FAKE + 4); add(fn, "norms-misaligned", norms=FAKE + 2)
    add(fn, "bad-shape+null", norms=None, **two)
    for fn in ("cmlpl_train_step", "cmlpl_train_step_opt"):
        nulls(fn, ("shape", "hp", "io"))
        for f in ("d_workspace", "d_params", "d_grads", "d_packed", "d_logits", "d_feat", "d_scalars", "d_labels", "d_m",
                  "d_v", "d_xl", "d_xu", "d_xpl", "d_xpu"):
            add(fn, f"io-null-{f}", io={f: None})
        add(fn, "bad-shape", shape=BAD); add(fn, "no-route", shape=NOROUTE)
        add(fn, "bt-0", io=dict(bt=0)); add(fn, "btu-0", io=dict(btu=0))
        add(fn, "reserved-bit-10", io=dict(reserved=1 << 10)); add(fn, "method-2", io=dict(reserved=2))
        add(fn, "sym-3", io=dict(reserved=3 << 8)); add(fn, "sym-without-cube", io=dict(reserved=1 << 8))
        add(fn, "cps-sym-without-cube", io=dict(reserved=1 | 2 << 8))
        add(fn, "dyn-table-without-cursor", io=dict(d_dyn_table=FAKE))
        add(fn, "dyn-cursor-without-table", io=dict(d_dyn_cursor=FAKE))
        add(fn, "dropout-1", hp=dict(dropout_p=1.0)); add(fn, "dropout-neg", hp=dict(dropout_p=-0.25))
        add(fn, "cube-with-rows", io=dict(d_cube=FAKE, cube_rows=32, cube_cols=32, d_lab_pix=FAKE, d_unl_pix=FAKE))
        add(fn, "cube-too-small", io=dict(d_xpl=None, d_xpu=None, d_cube=FAKE, cube_rows=5, cube_cols=32, d_lab_pix=FAKE,
                                          d_unl_pix=FAKE))
        add(fn, "ws-short", io_ws="step")
        add(fn, "ws-enough-for-the-passes-only", io_ws="pass")
        add(fn, "bad-shape+null", hp=None, **two); add(fn, "bad-shape+io-null", io=dict(d_grads=None), **two)
        add(fn, "no-route+io-null", shape=NOROUTE, io=dict(d_grads=None))
        add(fn, "no-route+bad-batch", shape=NOROUTE, io=dict(d_xl=None))
        add(fn, "io-null+ws-short", io=dict(d_feat=None), io_ws="step")
        add(fn, "bt-0+ws-short", io=dict(bt=0, workspace_bytes=0))
        add(fn, "reserved+ws-short", io=dict(reserved=1 << 10), io_ws="step")
        # what cmlpl_train_step itself does not look at comes after its workspace check
        add(fn, "bad-batch+ws-short", io=dict(d_xl=None), io_ws="step")
        add(fn, "dropout-1+ws-short", hp=dict(dropout_p=1.0), io_ws="step")
        add(fn, "dyn-table-without-cursor+ws-short", io=dict(d_dyn_table=FAKE), io_ws="step")
        add(fn, "dyn-table-without-cursor+bad-batch", io=dict(d_dyn_table=FAKE, d_xu=None))
        if fn.endswith("_opt"):
            for tag, o in bad_opts.items():
                add(fn, "opt-" + tag, opt=o)
            add(fn, "opt-decay-kills-weights", **kills)
            add(fn, "bad-opt+ws-short", opt=dict(max_norm=-1.0), io_ws="step")
            add(fn, "bad-opt+bad-shape", opt=dict(max_norm=-1.0), **two)
            add(fn, "bad-opt+io-null", opt=dict(max_norm=-1.0), io=dict(d_logits=None))
    for fn in ("cmlpl_step_graph_create", "cmlpl_step_graph_create_opt"):
        dyn = dict(d_dyn_table=FAKE, d_dyn_cursor=FAKE)
        add(fn, "null-io", io=None); add(fn, "null-graph_out", io=dyn, graph_out=None)
        add(fn, "no-dyn", io={}); add(fn, "no-cursor", io=dict(d_dyn_table=FAKE)); add(fn, "no-table", io=dict(d_dyn_cursor=FAKE))
        add(fn, "no-dyn+bad-shape", io={}, **two)
    fn = "cmlpl_dist_stage_graph_create"
    nulls(fn, ("shape", "hp", "dio", "graph_out"))
    add(fn, "no-table", dio=dict(d_dyn_table=None)); add(fn, "no-cursor", dio=dict(d_dyn_cursor=None))
    add(fn, "no-lab-idx", dio=dict(batch=dict(d_lab_idx=None))); add(fn, "no-unl-idx", dio=dict(batch=dict(d_unl_idx=None)))
    add(fn, "explicit-noise", dio=dict(batch=dict(noise8=C.cast(C.c_void_p(FAKE), C.POINTER(C.c_void_p)))))
    add(fn, "no-table+bad-stage", dio=dict(d_dyn_table=None), stage=99)
    fn = "cmlpl_debug_region"
    nulls(fn, ("shape", "name", "off", "size"))
    add(fn, "bad-shape", shape=BAD); add(fn, "no-route", shape=NOROUTE); add(fn, "nets-0", nets=0); add(fn, "nets-3", nets=3)
    add(fn, "n-0", n=0); add(fn, "unknown", name=b"nothing")
    for nm in (b"xn", b"probs", b"cps_pseudo"):
        add(fn, "one-net-" + nm.decode(), nets=1, name=nm)
    add(fn, "bad-shape+null", name=None, **two); add(fn, "no-route+null", shape=NOROUTE, off=None)
    add(fn, "no-route+unknown", shape=NOROUTE, name=b"nothing")
    assert len({r[0] for r in rows}) == len(rows)
    return rows


ROWS = _rows()


def collect(lib):
    """everything the fixture holds, from `lib`"""
    sizes = {size_key(*c): sizes_of(lib, *c) for c in size_cases()}
    refusals = {}
    for rid, fn, over in ROWS:
        rc = call(lib, fn, over)
        if not -3 <= rc <= -1:
            raise AssertionError(f"{rid}: the reference answers {rc}: not a refusal, the row does not belong in the table")
        refusals[rid] = rc
    return {"sizes": sizes, "refusals": refusals}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from cmlpl_amd import _lib
    lib = _lib.load()
    lib.cmlpl_debug_reload_switches()      # the record holds the default switches
    return lib


def test_the_tables_are_the_recorded_ones(golden):
    assert sorted(golden["sizes"]) == sorted(size_key(*c) for c in size_cases())
    assert sorted(golden["refusals"]) == sorted(r[0] for r in ROWS)
    assert all(-3 <= rc <= -1 for rc in golden["refusals"].values())


@pytest.mark.parametrize("case", size_cases(), ids=lambda c: size_key(*c))
def test_sizes_offsets_and_plans_are_the_parents(case, lib, golden):
    assert sizes_of(lib, *case) == golden["sizes"][size_key(*case)]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_refusal_is_the_parents(row, lib, golden):
    rid, fn, over = row
    assert call(lib, fn, over) == golden["refusals"][rid]


if __name__ == "__main__":
    from cmlpl_amd import _lib
    if not os.environ.get("CMLPL_LIB"):
        raise SystemExit("name the reference build with CMLPL_LIB: the record is not taken from the tree under test")
    record = collect(_lib.load())
    with open(FIXTURE, "w") as f:
        json.dump(record, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(ROWS), "refusals")
