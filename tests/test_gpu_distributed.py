"""GPU: the sample-sharded data-parallel step (cmlpl_amd.distributed) against the single-GPU step on
the same GLOBAL batch.  W ranks are emulated in one process on one GPU: every stage runs for all ranks,
then the collective that follows it is performed on the ranks' buffers (the real multi-process wiring of
the same stages is covered on CPU/gloo in test_distributed_gloo.py)."""
import copy

import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.gpu_util import DEV, cuda_batch, report, report_params, to_hp, to_shape
from tests.memo import memo, tensor_key

pytestmark = pytest.mark.gpu
SCALARS = ("ctr_s", "total_s", "cls_s", "con_s", "acc", "total_w", "cls_w", "con_w", "ctr_w",
           "n_mask_w", "n_mask_s", "n_pos", "n_neg")


class FakeComm:
    def __init__(self, world, rank):
        self.world, self.rank = world, rank


def _exchange(engines, stage):
    """the collectives that follow `stage`, performed on the ranks' buffers right away (every rank's stage has been
    enqueued on the one stream, so also an exchange the product issues asynchronously finds its input in stream order)"""
    W = len(engines)
    specs = [e.exchange_after(stage) for e in engines]
    for k in range(len(specs[0])):
        kind = specs[0][k][0]
        if kind == "all_gather":
            full = torch.cat([specs[r][k][2].reshape(-1) for r in range(W)])
            for r in range(W):
                specs[r][k][1].view(-1).copy_(full)
        elif kind == "reduce_scatter":
            tot = sum(specs[r][k][2] for r in range(W))
            for r, chunk in enumerate(tot.chunk(W, dim=0)):
                specs[r][k][1].copy_(chunk)
        else:
            tot = sum(specs[r][k][1] for r in range(W))
            for r in range(W):
                specs[r][k][1].copy_(tot)


def lockstep_step(engines, per_rank_inputs, epoch, batch_index, **kw):
    first = engines[0].STAGES[0]
    for e, inp in zip(engines, per_rank_inputs):
        getattr(e, "stage_" + first)(*inp["args"], epoch, batch_index, noise=inp.get("noise"), dropmask=inp.get("dropmask"), **kw)
    for stage in engines[0].STAGES:
        if stage != first:
            for e in engines:
                getattr(e, "stage_" + stage)()
        _exchange(engines, stage)


def global_outputs(engines, which):
    """(logits, feat) of the global batch as rank `which` sees them; the step never gathers the logits, the harness hands
    the ranks' blocks over"""
    full = torch.cat([e.logits_l.reshape(-1) for e in engines])
    return engines[which].outputs(gathered_logits=full)


def shard_inputs(cb, W, bt, btu, cls_in, with_noise):
    out = []
    bl, bul = bt // W, btu // W
    for r in range(W):
        ls, us = slice(r * bl, (r + 1) * bl), slice(r * bul, (r + 1) * bul)
        d = dict(args=(cb["XPl"][ls].contiguous(), cb["Xl"][ls].contiguous(), cb["Y"][ls].contiguous(),
                       cb["XPu"][us].contiguous(), cb["Xu"][us].contiguous()))
        if with_noise:
            nz = cb["noise"]
            d["noise"] = [nz[0][ls].contiguous(), nz[1][ls].contiguous(), nz[2][ls].contiguous(), nz[3][ls].contiguous(),
                          nz[4][us].contiguous(), nz[5][us].contiguous(), nz[6][us].contiguous(), nz[7][us].contiguous()]
            dm = cb["dropmask"]      # [2][n][F], rows [labelled ; unlabelled]
            d["dropmask"] = torch.cat([dm[:, ls], dm[:, bt:][:, us]], dim=1).contiguous()
        out.append(d)
    return out


@pytest.mark.parametrize("W,shape_name,bt,btu,explicit", [(2, "B2", 32, 32, True), (4, "B2", 64, 64, True),
                                                          (2, "P", 16, 16, True), (2, "B2", 64, 64, False),
                                                          (8, "B2", 64, 128, False), (2, "K40", 16, 16, True)])
def test_sharded_step_equals_single_gpu_step(W, shape_name, bt, btu, explicit):
    from cmlpl_amd import TrainEngine
    from cmlpl_amd.distributed import DistTrainEngine
    # K40: more than 32 classes on a small window -- the packed-buffer readers meet pair_exp_kernel's shuffle epilogue
    shape = {"B2": O.NetShape(103, 11, 11, 103, 9), "P": O.NetShape(60, 20, 20, 103, 9),
             "K40": O.NetShape(16, 8, 8, 12, 40)}[shape_name]
    hp = O.HyperParams()
    p0, p1 = O.closed_form_params(shape, 31), O.closed_form_params(shape, 32)
    ref = TrainEngine(to_shape(shape), bt, btu, to_hp(hp), device=DEV, seed=99)
    engines = [DistTrainEngine(to_shape(shape), bt // W, btu // W, to_hp(hp), device=DEV, seed=99, comm=FakeComm(W, r))
               for r in range(W)]
    for e in [ref] + engines:
        e.load_state_dict(0, p0); e.load_state_dict(1, p1)
    assert engines[0].Q == ref.Q
    for s in range(4):
        b = O.synthetic_batch(shape, bt, btu, 900 + s, separable=1.0 if s >= 2 else 0.0)
        cb = cuda_batch(b)
        epoch = 1          # smoothing active from the first step
        if explicit:
            ref.step(cb["XPl"], cb["Xl"], cb["Y"], cb["XPu"], cb["Xu"], epoch, s, noise=cb["noise"], dropmask=cb["dropmask"])
        else:
            ref.step(cb["XPl"], cb["Xl"], cb["Y"], cb["XPu"], cb["Xu"], epoch, s)
        lockstep_step(engines, shard_inputs(cb, W, bt, btu, shape.cls_in, explicit), epoch, s)
        torch.cuda.synchronize()
        want = ref.read_scalars()
        got_t = sum(e.scalars for e in engines)                      # shares are additive
        got = dict(zip(want.keys(), got_t.tolist()))
        print(f"step {s}: W={W} got={ {k: round(v, 6) for k, v in got.items()} }")
        for k in ("ctr_s", "total_s", "cls_s", "con_s", "acc", "total_w", "cls_w", "con_w"):
            assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]) + 1e-6, (s, k, got[k], want[k])
        assert [got[k] for k in ("n_mask_w", "n_mask_s", "n_pos", "n_neg")] == \
               [want[k] for k in ("n_mask_w", "n_mask_s", "n_pos", "n_neg")]
        lo, fe = ref.outputs()
        report("logits_g", global_outputs(engines, 0)[0], lo, 1e-5, 1e-5)     # same kernels; only the tile grouping differs
        report("feat_g", global_outputs(engines, -1)[1], fe, 1e-5, 5e-6)     # after updates: fp32 reduction-order drift
        for net in range(2):
            for k in O.LIVE_KEYS:
                gr = ref.grad(net, k)
                mx = max(float(gr.abs().max()), 1e-6)
                for e in (engines[0], engines[-1]):
                    report(f"grad[{net}] {k}", e.grad(net, k), gr, 2e-4, 2e-5 * mx)
        for i in range(2):
            for e in (engines[0], engines[-1]):
                report(f"bank{i} feats", e.bank_feats[i], ref.bank_feats[i], 1e-5, 5e-6)
                report(f"bank{i} probs", e.bank_probs[i], ref.bank_probs[i], 1e-5, 5e-6)
        assert engines[0].ptr == ref.ptr
        # parameters after this step's Adam update (one update from equal states; an element whose gradient is ~eps
        # may move by O(lr) on a rounding-level difference of the all-reduced sum, see report_params) ...
        for net in range(2):
            sd_ref = ref.state_dict(net)
            for e in (engines[0], engines[-1]):
                sd = e.state_dict(net)
                for k in O.LIVE_KEYS:
                    report_params(f"param[{net}] {k}", sd[k], sd_ref[k], 1, hp.lr)
        # every replica holds the same parameters bit for bit (same all-reduced gradient, same Adam)
        for e in engines[1:]:
            assert torch.equal(e.params, engines[0].params)
        # ... and every step is compared from EQUAL states: the sharded engines continue from the single-GPU
        # engine's parameters, Adam moments and banks.  (Left to themselves the two trajectories drift apart like any
        # two runs whose gradient sums differ in the last bit: by step 3 of B2 / 64+64 a near-zero-gradient weight of
        # conv0 had moved, and a fifth of conv0's gradient elements differed by 1e-3 relative.)
        for e in engines:
            e.params.copy_(ref.params); e.m.copy_(ref.m); e.v.copy_(ref.v)
            e._packed_dirty = True
            for i in range(2):
                e.bank_feats[i].copy_(ref.bank_feats[i]); e.bank_probs[i].copy_(ref.bank_probs[i])


def test_sharded_trajectory_left_alone_stays_within_the_drift_bound():
    """Eight steps, W = 2, WITHOUT putting the sharded engines back on the single-GPU engine's state: the two runs are
    the same arithmetic up to the order in which fp32 gradient sums are formed (rank-local partial sums + all-reduce
    against one sum), and Adam turns a last-bit difference of a near-zero gradient into an O(lr) parameter difference
    (update ~ lr * sign(g)).  Stated bounds for this configuration (B2, 32 + 32 rows, explicit noise / dropout, lr 5e-4):
      every parameter within 2 * lr * steps of the single-GPU run (the worst case of the sign argument),
      at most 2 % of the elements of any tensor beyond 1e-4 + 1e-3 |w|,
      the logged scalars within 1e-2 relative at every step,
      the threshold / graph counts equal at step 0 (later steps may move a borderline sample);
    the measured drift is printed per step."""
    from cmlpl_amd import TrainEngine
    from cmlpl_amd.distributed import DistTrainEngine
    W, bt, btu, steps = 2, 32, 32, 8
    shape = O.NetShape(103, 11, 11, 103, 9)
    hp = O.HyperParams()
    p0, p1 = O.closed_form_params(shape, 31), O.closed_form_params(shape, 32)
    ref = TrainEngine(to_shape(shape), bt, btu, to_hp(hp), device=DEV, seed=99)
    engines = [DistTrainEngine(to_shape(shape), bt // W, btu // W, to_hp(hp), device=DEV, seed=99, comm=FakeComm(W, r))
               for r in range(W)]
    for e in [ref] + engines:
        e.load_state_dict(0, p0); e.load_state_dict(1, p1)
    worst = 0.0
    for s in range(steps):
        b = O.synthetic_batch(shape, bt, btu, 1900 + s, separable=1.0 if s >= 2 else 0.0)
        cb = cuda_batch(b)
        ref.step(cb["XPl"], cb["Xl"], cb["Y"], cb["XPu"], cb["Xu"], 1, s, noise=cb["noise"], dropmask=cb["dropmask"])
        lockstep_step(engines, shard_inputs(cb, W, bt, btu, shape.cls_in, True), 1, s)
        torch.cuda.synchronize()
        want = ref.read_scalars()
        got = dict(zip(want.keys(), sum(e.scalars for e in engines).tolist()))
        rel = max(abs(got[k] - want[k]) / (abs(want[k]) + 1e-6) for k in ("ctr_s", "total_s", "cls_s", "total_w", "cls_w"))
        pmax, frac = 0.0, 0.0
        for net in range(2):
            for k in O.LIVE_KEYS:
                a, r_ = engines[0].view(engines[0].params, net, k), ref.view(ref.params, net, k)
                d = (a - r_).abs()
                pmax = max(pmax, float(d.max()))
                frac = max(frac, float((d > 1e-4 + 1e-3 * r_.abs()).float().mean()))
        print(f"step {s}: scalar drift {rel:.2e}  max |param diff| {pmax:.2e} (bound {2 * hp.lr * (s + 1):.1e})  "
              f"worst tensor fraction outside 1e-4 + 1e-3|w|: {frac:.4f}")
        worst = max(worst, rel)
        assert rel <= 1e-2, (s, rel)
        assert pmax <= 2 * hp.lr * (s + 1) + 1e-6, (s, pmax)
        assert frac <= 0.02, (s, frac)
        if s == 0:
            assert [got[k] for k in ("n_mask_w", "n_mask_s", "n_pos", "n_neg")] == \
                   [want[k] for k in ("n_mask_w", "n_mask_s", "n_pos", "n_neg")]
        assert engines[0].ptr == ref.ptr
        for e in engines[1:]:
            assert torch.equal(e.params, engines[0].params)          # replicas never diverge from each other
    print(f"worst scalar drift over {steps} steps without re-synchronisation: {worst:.2e}")


def _global_gates(engines, shape, bt_l, btu_l):
    """ReLU decisions of all ranks in GLOBAL row order [labelled of all ranks ; unlabelled of all ranks]."""
    from tests.gpu_util import hip_relu_gates
    per_rank = [hip_relu_gates(e, shape, bt_l + btu_l) for e in engines]
    out = []
    for net in range(2):
        g = {}
        for key in ("z1", "z2", "zy"):
            g[key] = torch.cat([pr[net][key][:bt_l] for pr in per_rank] + [pr[net][key][bt_l:] for pr in per_rank])
        out.append(g)
    return out


def _gate_tensors(g):
    """every tensor of a (nested) relu_gates structure, in a fixed order"""
    if torch.is_tensor(g):
        return [g]
    if isinstance(g, dict):
        return [t for k in sorted(g) for t in _gate_tensors(g[k])]
    if isinstance(g, (list, tuple)):
        return [t for v in g for t in _gate_tensors(v)]
    return []


def _detached(o):
    if torch.is_tensor(o):
        return o.detach()
    if isinstance(o, dict):
        return type(o)((k, _detached(v)) for k, v in o.items())
    if isinstance(o, (list, tuple)):
        return type(o)(_detached(v) for v in o)
    return o


@pytest.mark.parametrize("cfg", ["B3", "B5"])
def test_eight_rank_baseline_configs_match_the_oracle(cfg):
    """BASELINE.json configs[2] and configs[4] as they are sharded over 8 GPUs, each rank's stages run in lockstep
    on this one GPU, compared with the ORACLE on the global batch (not with the single-GPU engine):
      B3: PaviaU shape 11x11x103, global 512+512 -> 64+64 rows per rank, peaky regime so that thresholds, pos/neg
          masks and the mutual loss fire across shard boundaries;
      B5: 15x15x48, 20 classes, global 64+512 (1:8) -> 8+64 rows per rank.  n = 576 rows meet a 640-row bank with a
          256-row pointer step: from the second step on the writes wrap modulo Q and overlap the previous step's
          rows (the reference's slice-assign raises there -- SURVEY.md D5; the documented generalisation is
          tested against the oracle's modulo write).  Step 0 is also held to the reference's own numbers
          (tests/golden/b5_1to8.npz, the one step the reference can run at this split)."""
    from cmlpl_amd.distributed import DistTrainEngine
    from tests.golden_util import GoldenCase, rel_err
    from tests.gpu_util import relu_mask_audit
    W = 8
    if cfg == "B3":
        shape, bt, btu, steps, epoch = O.NetShape(103, 11, 11, 103, 9), 512, 512, 3, 12
        hp = O.HyperParams(thr=0.9)
        p0, p1 = O.closed_form_params(shape, 41), O.closed_form_params(shape, 42)
        for p in (p0, p1):
            p["classifier.weight"] *= 30.0
        batch = lambda s: O.synthetic_batch(shape, bt, btu, 4100 + s, separable=1.5)
        gold = None
    else:
        gold = GoldenCase("b5_1to8")
        shape, bt, btu, steps, epoch, hp = gold.shape, gold.bt, gold.btu, 4, gold.epoch0, gold.hp
        p0, p1 = gold.params()
        batch = gold.batch
    bt_l, btu_l = bt // W, btu // W
    st = O.StepState.create(shape, p0, p1, bt, hp)
    engines = [DistTrainEngine(to_shape(shape), bt_l, btu_l, to_hp(hp), device=DEV, seed=7, comm=FakeComm(W, r))
               for r in range(W)]
    for e in engines:
        e.load_state_dict(0, p0); e.load_state_dict(1, p1)
    assert engines[0].Q == st.bank_feats[0].shape[0] == 10 * bt
    fired = 0
    chain = ""
    for s in range(steps):
        b = batch(s)
        cb = cuda_batch(b)
        lockstep_step(engines, shard_inputs(cb, W, bt, btu, shape.cls_in, True), epoch, s)
        torch.cuda.synchronize()
        gates = _global_gates(engines, shape, bt_l, btu_l)
        # (the oracle's step on the 1024-row global batch is what this test's time goes into; the kernel variants walked by
        #  tests/test_gpu_env_paths.py in one process meet the same inputs and -- almost always -- the same ReLU decisions:
        #  the step is then taken from the in-process memo together with the state it leaves behind)
        chain = f"{chain}|{s}:{tensor_key(*_gate_tensors(gates))}"

        def oracle_step():
            r = O.train_step(st, b["XPl"], b["Xl"], b["Y"], b["XPu"], b["Xu"], b["noise"], b["dropmask"], epoch, s, hp,
                             relu_gates=gates)
            return _detached(r), copy.deepcopy(st)
        ref, st_after = memo(f"eight-rank-{cfg}-{chain}", oracle_step, disk=False)
        st.__dict__.update(copy.deepcopy(st_after).__dict__)
        got = dict(zip(SCALARS, sum(e.scalars for e in engines).tolist()))      # shares are additive
        want = dict(ctr_s=ref["ctr_s"], total_s=ref["total_s"], cls_s=ref["cls_s"], con_s=ref["con_s"], acc=ref["acc"],
                    total_w=ref["total_w"], cls_w=ref["cls_w"], con_w=ref["con_w"], ctr_w=ref["ctr_w"])
        want = {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in want.items()}
        print(f"[{cfg}] step {s}: " + " ".join(f"{k}={got[k]:.6g}/{v:.6g}" for k, v in want.items()))
        for k, v in want.items():
            assert abs(got[k] - float(v)) <= 1e-4 * abs(float(v)) + 1e-6, (s, k, got[k], float(v))
        assert [got["n_mask_w"], got["n_mask_s"], got["n_pos"], got["n_neg"]] == \
               [float(ref["mask_w"].sum()), float(ref["mask_s"].sum()), ref["n_pos"], ref["n_neg"]]
        fired += int(ref["mask_w"].sum()) + int(ref["mask_s"].sum())
        if gold is not None and s == 0:      # the reference's own step at 64+512
            z = gold.z
            row = [got[k] for k in ("ctr_s", "total_s", "cls_s", "con_s", "acc")]
            assert rel_err(row, z["hist"][0], 1e-7) < 1e-4, (row, z["hist"][0])
            assert rel_err([got[k] for k in ("total_w", "cls_w", "con_w", "ctr_w")], z["extra"][0], 1e-7) < 1e-4
            assert [got["n_mask_w"], got["n_mask_s"], got["n_pos"], got["n_neg"]] == list(z["counts"][0])
            assert engines[0].ptr == [int(v) for v in z["ptr"][0]]
            report("golden logits", global_outputs(engines, 0)[0], z["s0_logits"], 2e-4, 5e-5)
        lo_ref = torch.stack(ref["logits"])
        report("logits_g", global_outputs(engines, 0)[0], lo_ref, 2e-4, 5e-6 * float(lo_ref.abs().max()) + 2e-5)
        report("feat_g", global_outputs(engines, -1)[1], torch.stack(ref["feats"]), 1e-5, 3e-6)
        for r, e in enumerate(engines):      # every rank's masks sit on the oracle's signs (its own rows)
            rows = list(range(r * bt_l, (r + 1) * bt_l)) + list(range(bt + r * btu_l, bt + (r + 1) * btu_l))
            taps = [{k: v[rows] for k, v in ref["taps"][net].items()} for net in range(2)]
            # (after s Adam updates the boundary widens as in tests/test_gpu_step.py: a weight with an eps-sized gradient may
            #  sit O(lr) away from the oracle's)
            relu_mask_audit(e, taps, shape, bt_l + btu_l, ztol=2e-5 + 0.1 * hp.lr * s, ztol_y=2e-5 + 0.25 * hp.lr * s)
        for net in range(2):
            for k in O.LIVE_KEYS:
                gr = ref["grads"][net][k]
                mx = max(float(gr.abs().max()), 1e-4)
                for e in (engines[0], engines[-1]):     # all-reduced: every rank holds the global gradient
                    report(f"grad[{net}] {k}", e.grad(net, k), gr, 5e-4, 5e-5 * mx)
        assert engines[0].ptr == list(st.ptr)
        for i in range(2):
            for e in (engines[0], engines[-1]):
                report(f"bank{i} feats", e.bank_feats[i], st.bank_feats[i], 1e-5, 5e-6)
                report(f"bank{i} probs", e.bank_probs[i], st.bank_probs[i], 1e-4, 2e-4)
    if cfg == "B3":
        assert fired > 0          # the thresholds did fire in this regime
    for net in range(2):
        for e in (engines[0], engines[-1]):
            sd = e.state_dict(net)
            for k in O.LIVE_KEYS:
                report_params(f"param[{net}] {k}", sd[k], st.params[net][k], steps, hp.lr)
    for e in engines[1:]:
        assert torch.equal(e.params, engines[0].params)       # replicas stay bit-identical


def _dist_state(e):
    return [e.params.clone(), e.m.clone(), e.v.clone(), e.grads.clone(), e.bank_feats.clone(), e.bank_probs.clone(),
            e.scalar_hist.clone()]


@pytest.mark.parametrize("W,name,bt_l,btu_l", [(1, "B2", 64, 64), (2, "B2", 24, 40), (2, "B5", 8, 64), (1, "P", 16, 16)])
def test_replayed_stage_graphs_are_bit_identical_to_the_eager_sharded_step(W, name, bt_l, btu_l):
    """DistStepGraph -- the five stages of the sharded step as captured graphs, every per-step scalar from the device
    table, the exchanges in between -- against the eager sharded step by index: parameters, Adam moments, gradient
    bucket, banks and logged rows BIT-identical on every rank over a schedule that crosses the smoothing gate (batch 17
    -> 18 of epoch 0) and two epoch boundaries (W ranks in lockstep on this GPU; W = 1: the aliased one-rank engine)."""
    from cmlpl_amd import HyperParams, NetShape
    from cmlpl_amd.distributed import DistTrainEngine, NoOpComm
    shapes = {"B2": (103, 11, 11, 103, 9), "B5": (48, 15, 15, 48, 20), "P": (60, 20, 20, 103, 9)}
    C, H, Wd, bands, K = shapes[name]
    g = torch.Generator().manual_seed(17)
    NL, NU = 4 * bt_l * W + 3, 4 * btu_l * W + 5
    XP = torch.randn(NL, C, H, Wd, generator=g).to(DEV); X = torch.randn(NL, bands, generator=g).to(DEV)
    Y = torch.randint(0, K, (NL,), generator=g).to(DEV)
    XPu = torch.randn(NU, C, H, Wd, generator=g).to(DEV); Xu = torch.randn(NU, bands, generator=g).to(DEV)
    lab_perm = torch.randperm(NL, generator=g).to(DEV); unl_perm = torch.randperm(NU, generator=g).to(DEV)
    sched = [(0, 16), (0, 17), (0, 18), (0, 19), (1, 0), (1, 1), (2, 0)]
    offs = [((k % 4) * bt_l * W, (k % 4) * btu_l * W) for k in range(len(sched))]     # global offsets of step k's batch

    def make():
        es = [DistTrainEngine(NetShape(*shapes[name]), bt_l, btu_l, HyperParams(), device=DEV, seed=1088,
                              comm=(NoOpComm() if W == 1 else FakeComm(W, r)), hist_rows=8) for r in range(W)]
        for e in es:
            e.init_params_default(1088)
        return es

    def eager(es, k):
        ep, bi = sched[k]
        for r, e in enumerate(es):
            lo, uo = offs[k][0] + r * bt_l, offs[k][1] + r * btu_l
            e.stage_spectral(XP, X, Y, XPu, Xu, ep, bi, lab_idx=lab_perm[lo:lo + bt_l], unl_idx=unl_perm[uo:uo + btu_l])
        for stage in es[0].STAGES:
            if stage != "spectral":
                for e in es:
                    getattr(e, "stage_" + stage)()
            if W > 1:
                _exchange(es, stage)

    ea, eb = make(), make()
    for k in range(len(sched)):
        eager(ea, k)
    eager(eb, 0)                                                     # warm-up step, then everything from the graphs
    graphs = [e.capture(XP, X, Y, XPu, Xu, lab_perm, unl_perm, bt_l, btu_l, capacity=8) for e in eb]
    for r, gr in enumerate(graphs):
        gr.program([(sched[k][0], sched[k][1], offs[k][0] + r * bt_l, offs[k][1] + r * btu_l) for k in range(1, len(sched))])
    for k in range(1, len(sched)):
        for stage in eb[0].STAGES:
            for gr in graphs:
                gr.launch_stage(stage)
            if W > 1:
                _exchange(eb, stage)
    torch.cuda.synchronize()
    for r in range(W):
        assert ea[r].ptr == eb[r].ptr and ea[r].adam_t == eb[r].adam_t and ea[r].step_count == eb[r].step_count
        for i, (x, y) in enumerate(zip(_dist_state(ea[r]), _dist_state(eb[r]))):
            assert torch.equal(x, y), f"rank {r}: state tensor {i} differs, max |d| = {(x - y).abs().max().item():.3e}"
    assert torch.isfinite(eb[0].scalar_hist[:len(sched)]).all()
    with pytest.raises(RuntimeError):
        graphs[0].launch_stage("spectral")                           # nothing programmed
    for gr in graphs:
        gr.close()
