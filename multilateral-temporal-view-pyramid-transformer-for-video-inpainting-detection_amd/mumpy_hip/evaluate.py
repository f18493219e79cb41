"""Eval step of the reference (test.py:86-111 + measure.py:57-62,86-89) on device — SURVEY 8f-1.

    frames (uint8, optional) -> normalize_u8 -> Encoder -> Decoder.predict_mask (logits + thresholded uint8 mask from the
    same last kernel) -> per-clip F1 / IoU sums -> ONE all-reduce of the 3-float metric vector across ranks.
"""
import torch

from . import ops
from .distributed import all_reduce_metric, eval_metric_vector


@torch.no_grad()
def eval_step(encoder, decoder, x, gt_mask=None, thr=0.5):
    """x: (B,T,3,224,224) float32 clip, or (B,T,Hs,Ws,3) uint8 frames of any size (then the loader's resize to 224x224 --
    PIL NEAREST, universaldataset.py:75-79 -- and ToTensor+Normalize run on device in one kernel).
    Returns (mask uint8 (B,1,224,224), logits, metric_vector or None)."""
    if x.dtype == torch.uint8:
        x = ops.normalize_u8(x, size=(224, 224))
    fx, vx, dx = encoder(x)
    logits, mask, _ = decoder.predict_mask(fx, vx, dx, thr)
    metric = eval_metric_vector(mask, gt_mask) if gt_mask is not None else None
    return mask, logits, metric


def finalize_metrics(metric_sum: torch.Tensor):
    """All-reduce the accumulated [sum F1, sum IoU, n] vector (the path's only collective) -> (mean F1, mean IoU, n)."""
    v = all_reduce_metric(metric_sum.clone())
    n = float(v[2])
    return float(v[0]) / max(n, 1.0), float(v[1]) / max(n, 1.0), int(n)


def finalize_sweep(table, acc, pooled) -> dict:
    """What VideoPredictor.sweep_vector() returns -- table (K,) float32, acc (K, 3) float64 = per threshold [sum F1, sum IoU, n],
    pooled (2, K + 1) int64 = the exceed counts summed over the frames -- all-reduced across ranks as finalize_metrics does its vector
    (the identity without a process group), then on the host:
      thresholds, f1, iou   numpy arrays of length K: the table and the per-threshold means over the n frames;
      n                     the number of frames scored;
      best                  (threshold, f1, iou) at the highest mean F1; the lowest threshold wins a tie;
      auc                   the pixel-level area under the ROC curve through the table's points FPR_k = pooled[0][k] / pooled[0][K],
                            TPR_k = pooled[1][k] / pooled[1][K] and the end points (0, 0) and (1, 1), by the trapezoid rule in
                            fp64; nan when either class is empty.
    auc is the AUC AT THE TABLE'S RESOLUTION: the curve is known at the table's K operating points only and is taken as a straight
    line between two neighbours (and from the outermost ones to the corners); a finer table resolves more of it."""
    import numpy as np
    table = torch.as_tensor(table)
    acc, pooled = torch.as_tensor(acc), torch.as_tensor(pooled)
    k = table.numel()
    if table.dim() != 1 or k < 1 or tuple(acc.shape) != (k, 3) or tuple(pooled.shape) != (2, k + 1):
        raise ValueError(f"finalize_sweep: needs table (K,), acc (K, 3) and pooled (2, K + 1), got {tuple(table.shape)}, "
                         f"{tuple(acc.shape)} and {tuple(pooled.shape)}")
    a = all_reduce_metric(acc.to(torch.float64).clone()).cpu().numpy()
    p = all_reduce_metric(pooled.to(torch.int64).clone()).cpu().numpy().astype(np.float64)
    thr = table.detach().cpu().numpy().astype(np.float32)
    n = float(a[0, 2])
    f1, iou = a[:, 0] / max(n, 1.0), a[:, 1] / max(n, 1.0)
    b = int(np.argmax(f1))                                           # the first of equal maxima: the lowest threshold
    neg, pos = p[0, k], p[1, k]
    if neg > 0 and pos > 0:
        # thresholds ascend, so the rates descend: walk from (1, 1) at "below every threshold" to (0, 0) at "above every one"
        fpr = np.concatenate([[1.0], p[0, :k] / neg, [0.0]])
        tpr = np.concatenate([[1.0], p[1, :k] / pos, [0.0]])
        auc = float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) * 0.5))
    else:
        auc = float("nan")
    return dict(thresholds=thr, f1=f1, iou=iou, n=int(n), best=(float(thr[b]), float(f1[b]), float(iou[b])), auc=auc)
