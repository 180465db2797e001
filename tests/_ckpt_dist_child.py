"""Child of tests/test_gpu_checkpoint.py: one rank of a REAL two-process data-parallel job on ONE GPU (every rank uses
cuda:0, the collectives run on gloo -- as tests/_dist_gpu_child.py).  A W-rank DistTrainEngine pair runs 6 steps
straight; a second pair runs 3, rank 0 saves, a FRESH pair loads the file and runs the other 3: parameters, moments,
banks and logged rows must equal the straight pair's byte for byte on every rank.  Rank 0 then loads the same file into
a single-process TrainEngine that runs the same global batches beside another fresh pair: step by step they agree to the
tolerances of tests/_dist_gpu_child.py:95-106 (W ranks against one differ by fp32 summation order)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from cmlpl_amd import HyperParams, NetShape, TrainEngine, checkpoint  # noqa: E402
from cmlpl_amd.distributed import DistTrainEngine  # noqa: E402
from oracle import cmlpl_oracle as O  # noqa: E402  (input generators only)

rank, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
path = sys.argv[1]
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
dist.init_process_group("gloo")
oshape, shape = O.NetShape(103, 11, 11, 103, 9), NetShape(103, 11, 11, 103, 9)
bt, btu, STEPS, CUT = 32, 64, 6, 3
bl, bul = bt // W, btu // W
hp = HyperParams()
p0, p1 = O.closed_form_params(oshape, 51), O.closed_form_params(oshape, 52)
d = lambda t: t.to(dev).contiguous()
batches = [O.synthetic_batch(oshape, bt, btu, 800 + s, separable=1.0) for s in range(STEPS)]
sched = [(0, 15 + s) for s in range(STEPS)]            # crosses the smoothing gate (batch_index > queue_batch = 17)
ls, us = slice(rank * bl, (rank + 1) * bl), slice(rank * bul, (rank + 1) * bul)


def pair():
    e = DistTrainEngine(shape, bl, bul, hp, device=dev, seed=5, hist_rows=8)
    e.load_state_dict(0, p0); e.load_state_dict(1, p1)
    return e


def run(e, steps, rows=(ls, us)):
    a, b_ = rows
    for s in steps:
        b = batches[s]
        e.step(d(b["XPl"][a]), d(b["Xl"][a]), d(b["Y"][a]), d(b["XPu"][b_]), d(b["Xu"][b_]), sched[s][0], sched[s][1])


A = pair()
run(A, range(STEPS))
B = pair()
run(B, range(CUT))
if rank == 0:
    checkpoint.save(path, B.checkpoint_state(), dict(note="two ranks"))
dist.barrier()                                          # the file is complete before any rank reads it
ck = checkpoint.load(path)
Cn = DistTrainEngine(shape, bl, bul, hp, device=dev, seed=5, hist_rows=8)       # fresh: zero parameters
Cn.load_checkpoint_state(ck)
run(Cn, range(CUT, STEPS))
torch.cuda.synchronize()
for name in ("params", "m", "v", "bank_feats", "bank_probs"):
    x, y = getattr(A, name), getattr(Cn, name)
    assert torch.equal(x, y), f"rank {rank}: {name} differs after the resume, max |d| = {(x - y).abs().max().item():.3e}"
assert A.ptr == Cn.ptr and A.adam_t == Cn.adam_t and A.step_count == Cn.step_count == STEPS
assert torch.equal(A.scalar_hist[CUT:STEPS], Cn.scalar_hist[CUT:STEPS]), f"rank {rank}: logged rows differ"
assert torch.isfinite(Cn.scalar_hist[CUT:STEPS]).all()
# One process, the same file, the same GLOBAL batches.  Compared step by step from EQUAL states, as tests/_dist_gpu_child.py
# does (W ranks and one process differ by fp32 summation order, and Adam's normalised update amplifies that from one step
# to the next: tests/test_gpu_distributed.py), with its explicit noise / dropout masks and its tolerances.
D = DistTrainEngine(shape, bl, bul, hp, device=dev, seed=5)
D.load_checkpoint_state(ck)
one = None
if rank == 0:
    one = TrainEngine(shape, bt, btu, hp, device=dev, seed=5)
    one.load_checkpoint_state(ck)
for s in range(CUT, STEPS):
    b = batches[s]
    nz = b["noise"]
    noise = [d(nz[0][ls]), d(nz[1][ls]), d(nz[2][ls]), d(nz[3][ls]), d(nz[4][us]), d(nz[5][us]), d(nz[6][us]), d(nz[7][us])]
    dm = torch.stack([torch.cat([m[ls], m[bt:][us]]) for m in b["dropmask"]]).to(dev).contiguous()
    D.step(d(b["XPl"][ls]), d(b["Xl"][ls]), d(b["Y"][ls]), d(b["XPu"][us]), d(b["Xu"][us]), sched[s][0], sched[s][1],
           noise=noise, dropmask=dm)
    got = D.read_scalars()                              # all-reduced over the ranks
    if rank == 0:
        one.step(d(b["XPl"]), d(b["Xl"]), d(b["Y"]), d(b["XPu"]), d(b["Xu"]), sched[s][0], sched[s][1],
                 noise=[d(t) for t in nz], dropmask=torch.stack(b["dropmask"]).to(dev).contiguous())
        want = one.read_scalars()
        for k in ("ctr_s", "total_s", "cls_s", "con_s", "acc", "total_w", "cls_w", "con_w"):
            assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]) + 1e-6, (s, k, got[k], want[k])
        assert [got[k] for k in ("n_mask_w", "n_mask_s", "n_pos", "n_neg")] == [want[k] for k in ("n_mask_w", "n_mask_s", "n_pos", "n_neg")]
        for net in range(2):
            g, r = D.grads[net], one.grads[net, :D.live]
            err = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-9)
            assert err < 2e-4, (s, net, err)
        assert D.ptr == one.ptr and D.adam_t == one.adam_t and D.step_count == one.step_count
        for i in range(2):
            assert float((D.bank_feats[i] - one.bank_feats[i]).abs().max()) < 1e-5
            assert float((D.bank_probs[i] - one.bank_probs[i]).abs().max()) < 1e-5
    for name in ("params", "m", "v", "bank_feats", "bank_probs"):
        t = getattr(D, name)
        if rank == 0:
            t.copy_(getattr(one, name))
        dist.broadcast(t, 0)
    D._packed_dirty = True
if rank == 0:
    # a file of another global batch is refused by name
    small = TrainEngine(shape, bt // 2, btu, hp, device=dev, seed=5)
    try:
        small.load_checkpoint_state(ck)
        raise AssertionError("a checkpoint of another labelled batch was accepted")
    except ValueError as e:
        assert "bt:" in str(e) and "Q:" in str(e), str(e)
    print(f"OK checkpoint world={W}")
dist.barrier()
dist.destroy_process_group()
