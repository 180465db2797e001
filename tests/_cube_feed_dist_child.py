"""Child of tests/test_gpu_cube_feed_multiprocess.py: one rank of a REAL multi-process data-parallel job on ONE GPU (every
rank uses cuda:0, the collectives run on gloo -- as tests/_dist_gpu_child.py) whose sharded step is CUBE-FED: every rank
holds the scene cube and the whole splits' spectra / labels / pixel lists and takes its rows through index lists; rank 0
also runs the cube-fed single-process TrainEngine on the global batch and compares, within the bounds of the split-fed
sharded tests."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from cmlpl_amd import HyperParams, NetShape, TrainEngine  # noqa: E402
from cmlpl_amd.distributed import DistTrainEngine  # noqa: E402
from oracle import cmlpl_oracle as O  # noqa: E402  (parameter / noise generators only)

rank, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
dist.init_process_group("gloo")
shape = O.NetShape(103, 11, 11, 103, 9)
bt, btu, steps = 32, 64, 3
hp = HyperParams()
p0, p1 = O.closed_form_params(shape, 51), O.closed_form_params(shape, 52)
g = torch.Generator().manual_seed(21)                      # the same scene and splits on every rank
rows, cols = 23, 19
d = lambda t: t.to(dev).contiguous()
cube = d(torch.randn(rows, cols, 103, generator=g))
NL, NU = 3 * bt, 3 * btu
lab_pix, unl_pix = d(torch.randint(0, rows * cols, (NL,), generator=g)), d(torch.randint(0, rows * cols, (NU,), generator=g))
X, Y, Xu = d(torch.randn(NL, 103, generator=g)), d(torch.randint(0, 9, (NL,), generator=g)), d(torch.randn(NU, 103, generator=g))
src = dict(cube=cube, lab_pix=lab_pix, unl_pix=unl_pix)
eng = DistTrainEngine(NetShape(103, 11, 11, 103, 9), bt // W, btu // W, hp, device=dev, seed=5)
eng.load_state_dict(0, p0); eng.load_state_dict(1, p1)
ref = None
if rank == 0:
    ref = TrainEngine(NetShape(103, 11, 11, 103, 9), bt, btu, hp, device=dev, seed=5)
    ref.load_state_dict(0, p0); ref.load_state_dict(1, p1)
bl, bul = bt // W, btu // W
ls, us = slice(rank * bl, (rank + 1) * bl), slice(rank * bul, (rank + 1) * bul)
worst = 0.0
for s in range(steps):
    b = O.synthetic_batch(shape, bt, btu, 800 + s, separable=1.0)          # (its noise draws and dropout masks are used)
    nz = b["noise"]
    noise = [d(nz[0][ls]), d(nz[1][ls]), d(nz[2][ls]), d(nz[3][ls]), d(nz[4][us]), d(nz[5][us]), d(nz[6][us]), d(nz[7][us])]
    dm = torch.stack([torch.cat([m[ls], m[bt:][us]]) for m in b["dropmask"]]).to(dev).contiguous()
    li, ui = d(torch.randperm(NL, generator=g)[:bt]), d(torch.randperm(NU, generator=g)[:btu])      # the GLOBAL batch's rows
    eng.step(None, X, Y, None, Xu, 1, s, noise=noise, dropmask=dm, lab_idx=li[ls].contiguous(), unl_idx=ui[us].contiguous(), **src)
    got = eng.read_scalars()                       # all-reduced over the ranks
    if rank == 0:
        ref.step(None, X, Y, None, Xu, 1, s, noise=[d(t) for t in nz], dropmask=torch.stack(b["dropmask"]).to(dev).contiguous(),
                 lab_idx=li, unl_idx=ui, **src)
        want = ref.read_scalars()
        for k in ("ctr_s", "total_s", "cls_s", "con_s", "acc", "total_w", "cls_w", "con_w"):
            assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]) + 1e-6, (s, k, got[k], want[k])
        assert [got[k] for k in ("n_mask_w", "n_mask_s", "n_pos", "n_neg")] == [want[k] for k in ("n_mask_w", "n_mask_s", "n_pos", "n_neg")]
        live = eng.live
        for net in range(2):
            gr, r = eng.grads[net], ref.grads[net, :live]
            err = float((gr - r).abs().max()) / max(float(r.abs().max()), 1e-9)
            worst = max(worst, err)
            assert err < 2e-4, (s, net, err)
        assert eng.ptr == ref.ptr
        for i in range(2):
            assert float((eng.bank_feats[i] - ref.bank_feats[i]).abs().max()) < 1e-5
            assert float((eng.bank_probs[i] - ref.bank_probs[i]).abs().max()) < 1e-5
    # every step is compared from EQUAL states (as tests/_dist_gpu_child.py): all ranks continue from the single-process
    # engine's parameters, Adam moments and banks
    for name in ("params", "m", "v"):
        t = getattr(eng, name)
        if rank == 0:
            t.copy_(getattr(ref, name))
        dist.broadcast(t, 0)
    for i in range(2):
        for bank in (eng.bank_feats, eng.bank_probs):
            if rank == 0:
                bank[i].copy_((ref.bank_feats if bank is eng.bank_feats else ref.bank_probs)[i])
            dist.broadcast(bank[i], 0)
    eng._packed_dirty = True
if rank == 0:
    print(f"OK cube-fed world={W} steps={steps} worst_grad_rel_err={worst:.2e}")
dist.barrier()
dist.destroy_process_group()
