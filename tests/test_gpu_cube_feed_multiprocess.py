"""GPU: the CUBE-FED sharded step as two REAL processes (cmlpl_amd.launch.spawn_ranks -> torch.distributed rendezvous ->
DistTrainEngine + TorchDistComm, the ranks sharing cuda:0 with their collectives on gloo, as in
tests/test_gpu_multiprocess.py): W = 2 against the cube-fed single-process step on the global batch, within the bounds
the split-fed sharded tests use.  Three processes have the GPU open (the two ranks and this one)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cube_fed_sharded_step_equals_cube_fed_single_process():
    from cmlpl_amd.launch import spawn_ranks
    rc, out = spawn_ranks(2, [sys.executable, os.path.join(ROOT, "tests", "_cube_feed_dist_child.py")], timeout=600)
    assert rc == 0, out
    assert "OK cube-fed world=2" in out, out
