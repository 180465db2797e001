"""The seeded case of the ``test_acc`` fixture (tests/golden/make_golden_testacc.py records the reference's answer on it,
tests/test_eval_metrics.py runs this repository's ``tools.hyper_tools.test_acc`` on it)."""
import torch

NUM_CLASSES, N, BATCH, C, W, BANDS, EPOCH, PRINT_EVERY = 5, 236, 32, 3, 4, 7, 4, 2


class TinyNet(torch.nn.Module):
    """logits = spectrum . A + window mean . B, seeded; returns the logits alone, as the model the reference's test_acc
    was written for did (it takes torch.max of what the model returns)"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(77)
        self.A = torch.nn.Parameter(torch.randn(BANDS, NUM_CLASSES, generator=g, dtype=torch.float64))
        self.B = torch.nn.Parameter(torch.randn(C, NUM_CLASSES, generator=g, dtype=torch.float64))

    def forward(self, XP, X):
        return X.double() @ self.A + XP.double().mean((2, 3)) @ self.B


def case():
    """(model, loader of (XP, X, Y) batches): labels follow the model's own argmax on two thirds of the items, so the
    accuracy is neither 0 nor 1 and every class occurs; the last batch is short"""
    g = torch.Generator().manual_seed(1234)
    XP = torch.randn(N, C, W, W, generator=g)
    X = torch.randn(N, BANDS, generator=g)
    model = TinyNet()
    with torch.no_grad():
        pred = model(XP, X).argmax(1)
    rnd = torch.randint(0, NUM_CLASSES, (N,), generator=g)
    Y = torch.where(torch.rand(N, generator=g) < 2.0 / 3.0, pred, rnd)
    Y[:NUM_CLASSES] = torch.arange(NUM_CLASSES)
    ds = torch.utils.data.TensorDataset(XP, X, Y)
    return model, torch.utils.data.DataLoader(ds, batch_size=BATCH, shuffle=False)
