"""Caller-side helpers of the reference's tools/hyper_tools.py that the training driver uses around
the hot path: whole-image inference (hyper_tools.py:416-437), per-epoch validation (hyper_tools.py:372-413) and
OA / Kappa / per-class accuracy (hyper_tools.py:208-223).  Host-side glue only; the forward runs on the HIP kernels."""
import numpy as np
import torch


@torch.no_grad()
def test_whole(model, data_loader, print_per_batches=10):
    """argmax prediction for every pixel of the scene (reference hyper_tools.py:416-437).  ``data_loader`` yields
    (XP, X) batches of materialised patches, as in the reference -- or is a ``cmlpl_amd.infer.CubeSource`` (the scene
    cube [rows, cols, C] and the spectra, resident in HBM): the windows are then gathered on the device inside the
    forward kernel (cmlpl_infer_cube), no patch tensor and no DataLoader.  (The reference forgets no_grad here; the result
    is the same.)"""
    model.eval()
    from cmlpl_amd.infer import CubeSource, infer_cube
    if isinstance(data_loader, CubeSource):
        return infer_cube(model, data_loader.cube, data_loader.spectra).cpu().numpy()
    out = []
    for batch_idx, (XP, X) in enumerate(data_loader):
        logits, _ = model(XP.cuda(non_blocking=True), X.cuda(non_blocking=True))
        out.append(logits.argmax(1).cpu().numpy())
        if (batch_idx + 1) % print_per_batches == 0:
            print('---------------------Testing the whole set-[%d/%d]---------------------'
                  % (batch_idx + 1, len(data_loader)))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


@torch.no_grad()
def test_acc(model, data_loader, epoch, num_classes, print_per_batches=10):
    """Validation accuracy of one network after ``epoch`` (reference hyper_tools.py:372-413: same arguments, printed
    lines and return value -- the overall accuracy as a float; per-class accuracy and AA are printed).  ``data_loader``
    yields (XP, X, Y) batches as in the reference, or is a ``cmlpl_amd.evaluate.Evaluator`` (a split registered on the
    device): the forward is then list-fed from the scene cube, ``model`` is whatever ``infer_pixels`` takes for ONE network
    (a BaseNet2, or ``(TrainEngine, index)``), and the counts are the diagonal and the row sums of the confusion matrix
    counted on the device -- there are no batches, so no per-batch line.  A class without a validation sample divides
    by zero, as in the reference."""
    from cmlpl_amd.evaluate import Evaluator
    per_class = np.zeros((num_classes, 2))            # [class] = (correct, total)
    if isinstance(data_loader, Evaluator):
        cm = data_loader.evaluate(model)[0].cpu().numpy()[:num_classes]
        per_class[:, 0], per_class[:, 1] = np.diag(cm), cm.sum(1)
    else:
        model.eval()
        for batch_idx, (XP, X, Y) in enumerate(data_loader):
            out = model(XP.cuda(), X.cuda())
            logits = out[0] if isinstance(out, (tuple, list)) else out
            hit = (torch.max(logits, 1)[1].cpu() == Y.cpu()).double()
            lab = Y.cpu().reshape(-1).long()
            per_class[:, 0] += torch.bincount(lab, weights=hit, minlength=num_classes).numpy()
            per_class[:, 1] += torch.bincount(lab, minlength=num_classes).numpy()
            if (batch_idx + 1) % print_per_batches == 0:
                print('Epoch[%d]-Validation-[%d/%d] Batch OA: %.2f %%' % (
                    epoch, batch_idx + 1, len(data_loader), 100.0 * float(hit.sum()) / XP.size(0)))
    class_acc = np.zeros((num_classes, 1))
    for i in range(num_classes):
        class_acc[i] = 1.0 * float(per_class[i, 0]) / float(per_class[i, 1])
        print('---------------Accuracy of %5s : %.2f %%---------------' % (i, 100 * class_acc[i, 0]))
    acc = 1.0 * float(per_class[:, 0].sum()) / float(per_class[:, 1].sum())
    print('---------------Epoch[%d]Validation-OA: %.2f %%---------------' % (epoch, 100.0 * acc))
    print('---------------Epoch[%d]Validation-AA: %.2f %%---------------' % (epoch, 100.0 * np.mean(class_acc)))
    return acc


def CalAccuracy(predict, label):
    """OA, Kappa, producer's accuracy per class (confusion-matrix statistics)."""
    predict = np.asarray(predict).astype(np.int64)
    label = np.asarray(label).astype(np.int64)
    n = int(label.max()) + 1
    cm = np.zeros((n, n), dtype=np.float64)
    np.add.at(cm, (label, np.clip(predict, 0, n - 1)), 1.0)
    total = cm.sum()
    OA = np.trace(cm) / total
    pe = float((cm.sum(0) * cm.sum(1)).sum()) / (total * total)
    Kappa = (OA - pe) / (1.0 - pe) if pe < 1.0 else 0.0
    producerA = np.diag(cm) / np.maximum(cm.sum(1), 1.0)
    return OA, Kappa, producerA
