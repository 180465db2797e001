"""CPU: the restatement of the cross-pseudo-supervision step (tests/cps_util.py) against fixtures produced by the
reference's own step text (tests/golden/make_golden_cps.py, trian_CPS.py:188-258).  This is what pins the restatement."""
import numpy as np
import pytest
import torch

from oracle import cmlpl_oracle as O
from tests.cps_util import MARGIN_MIN, CpsCase, cps_cases, cps_step
from tests.golden_util import rel_err

RTOL = 2e-5      # the tolerance of tests/test_oracle_golden.py
FULL_PARAMS = ("conv0.bias", "conv1.bias", "conv2.bias", "classifier.bias")


def test_the_fixtures_cover_the_cases_the_method_was_pinned_on():
    names = cps_cases()
    assert {"cps_b2_32x3", "cps_p_16", "cps_b5_8to64"} <= set(names), names
    g = CpsCase("cps_b2_32x3")
    assert (g.bt, g.btu, g.steps) == (32, 32, 3) and g.shape == O.NetShape(103, 11, 11, 103, 9)
    g = CpsCase("cps_p_16")
    assert (g.bt, g.btu) == (16, 16) and g.shape == O.NetShape(60, 20, 20, 103, 9)       # the reference's own shape
    g = CpsCase("cps_b5_8to64")
    assert (g.bt, g.btu, g.shape.K) == (8, 64, 16)


@pytest.mark.parametrize("name", cps_cases())
def test_every_unlabelled_row_of_every_fixture_has_a_clear_argmax(name):
    """the condition the generator asserted on the reference's own logits: no row left out, both networks, every step"""
    g = CpsCase(name)
    z = g.z
    assert z["logits"].shape == (g.steps, 2, g.bt + g.btu, g.shape.K)
    top = np.sort(z["logits"][:, :, g.bt:, :].astype(np.float64), axis=-1)
    margins = top[..., -1] - top[..., -2]                    # [steps][2][btu]: every row
    assert margins.min() >= MARGIN_MIN, margins.min()
    assert abs(margins.min() - g.margin) <= 1e-12 + 1e-6 * g.margin
    assert np.array_equal(z["pseudo"][:, 0], z["logits"][:, 1, g.bt:].argmax(-1))       # Base learns Base1's label
    assert np.array_equal(z["pseudo"][:, 1], z["logits"][:, 0, g.bt:].argmax(-1))


@pytest.mark.parametrize("name", cps_cases())
def test_restatement_matches_reference_fixture(name):
    torch.set_num_threads(8)
    g = CpsCase(name)
    z = g.z
    p0, p1 = g.params()
    st = O.StepState.create(g.shape, p0, p1, g.bt, g.hp)
    banks0 = [t.clone() for t in st.bank_feats + st.bank_probs]
    for s in range(g.steps):
        out = cps_step(st, g.batch(s), g.hp)
        assert rel_err(out["hist"], z["hist"][s], 1e-9) < RTOL, (s, out["hist"], z["hist"][s])
        assert rel_err(out["extra"], z["extra"][s], 1e-9) < RTOL, (s, out["extra"], z["extra"][s])
        assert np.array_equal(out["pseudo"].numpy(), z["pseudo"][s]), s                    # exactly
        assert out["agree"] == int(z["agree"][s])
        assert np.allclose(torch.stack(out["logits"]).numpy(), z["logits"][s], rtol=1e-4, atol=2e-5)
        assert out["margin"] >= MARGIN_MIN
        for net in range(2):
            gn = [float(out["grads"][net][k].double().norm()) for k in O.LIVE_KEYS]
            assert rel_err(gn, z["grad_norms"][s][net], 1e-9) < 5e-5, (s, net, gn, z["grad_norms"][s][net])
            psum = [float(st.params[net][k].double().sum()) for k in O.LIVE_KEYS]
            assert np.allclose(psum, z["param_sums"][s][net], rtol=1e-5, atol=1e-5), (s, net)
            gc = out["grads"][net]["classifier.weight"].numpy()[:, :16]
            assert np.allclose(gc, z["grad_cls"][s][net], rtol=1e-4, atol=1e-6)
            pa = np.concatenate([st.params[net][k].numpy().reshape(-1) for k in FULL_PARAMS])
            assert np.allclose(pa, z["params_after"][s][net], rtol=1e-5, atol=1e-6), (s, net)
    # the method has no memory bank: the state's banks and pointers are as created
    assert all(torch.equal(a, b) for a, b in zip(banks0, st.bank_feats + st.bank_probs)) and list(st.ptr) == [0, 0]


def test_the_spectral_branch_is_reached_through_the_classifier_only():
    """no gradient enters the embedding (the step's d_dfeat is zero): scaling the embedding's share of the classifier
    input to zero must zero feat_spe's gradient"""
    g = CpsCase("cps_b5_8to64")
    p0, p1 = g.params()
    for p in (p0, p1):
        p["classifier.weight"][:, g.shape.spatial_feat:] = 0
    st = O.StepState.create(g.shape, p0, p1, g.bt, g.hp)
    out = cps_step(st, g.batch(0), g.hp, apply_update=False)
    for net in range(2):
        assert float(out["grads"][net]["feat_spe.weight"].abs().max()) == 0.0
        assert float(out["grads"][net]["conv1.weight"].abs().max()) > 0.0
