#!/usr/bin/env python3
"""Golden vector for tools.hyper_tools.test_acc: the reference's own ``test_acc`` (tools/hyper_tools.py:372-413) on the
seeded case of tests/testacc_util.py.

  * loads /root/reference/tools/hyper_tools.py BY PATH; `.cuda()` is patched to identity (CPU run);
  * stores DATA only (tests/golden/eval/testacc_ref.npz: a directory of its own, the step-trajectory tests take every .npz directly under tests/golden/): the returned accuracy, the per-class accuracies parsed back from the printed lines, and the
    printed lines themselves (as bytes).
Build container only:  python tests/golden/make_golden_testacc.py"""
import contextlib
import io
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden._refload import load_reference_module  # noqa: E402
from tests.testacc_util import EPOCH, NUM_CLASSES, PRINT_EVERY, case  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
ref = load_reference_module("tools/hyper_tools.py", "ref_hyper_tools", stubs=("torchvision", "hdf5storage", "scipy", "scipy.io", "sklearn", "sklearn.decomposition"))

model, loader = case()
buf = io.StringIO()
with contextlib.redirect_stdout(buf), torch.no_grad():
    acc = ref.test_acc(model, loader, EPOCH, NUM_CLASSES, print_per_batches=PRINT_EVERY)
lines = buf.getvalue()
per_class = [float(m) for m in re.findall(r"Accuracy of\s+\d+ : ([0-9.]+) %", lines)]
assert len(per_class) == NUM_CLASSES
np.savez(os.path.join(HERE, "eval", "testacc_ref.npz"), acc=np.array([acc], dtype=np.float64),
         per_class_percent=np.array(per_class, dtype=np.float64), printed=np.frombuffer(lines.encode(), dtype=np.uint8))
print(lines)
print("acc", acc)
