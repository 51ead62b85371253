"""Numpy float64 restatement of the semantic-evaluation contract (mu_sem_eval in include/maskunet_hip.h, maskunet_amd/metrics.py),
written from its definitions; nothing of maskunet_amd is used.  tests/test_semeval_host.py pins it to the reference-generated
fixtures and to scikit-learn before the GPU tests rely on it.

  pred      first maximum over the C real channels (np.argmax = torch.argmax);
  void      label == ignore, or outside [0, C);
  counts    per image I_c = #(pred == c and label == c), P_c = #(pred == c) over EVERY pixel, L_c = #(label == c);
  confusion [C+1, C]: row = label (C for void), column = pred;
  loss      per image {sum over the non-void rows of lse - x[label], number of such rows};
  prob      1 / sum_c exp((x_c - x_max) / temperature).
"""
import numpy as np

from tests._cc_reference import argmax_prob
from tests._loss_reference import ce_rows, iou_counts


def sem_eval(logits, labels, C, ignore, temperature=0.5):
    """logits [B, HW, >= C] ALREADY rounded to the dtype under test (only the first C channels are read), labels [B, HW] integers.
    Returns a dict: img_counts int64 [B,3,C], confusion int64 [C+1,C] (of this batch alone), img_loss float64 [B,2], cls int32
    [B,HW], prob float64 [B,HW]."""
    x = np.asarray(logits, np.float64)[:, :, :C]
    lab = np.asarray(labels, np.int64)
    B, HW = lab.shape
    assert x.shape[:2] == (B, HW)
    counts = np.zeros((B, 3, C), np.int64)
    conf = np.zeros((C + 1, C), np.int64)
    loss = np.zeros((B, 2), np.float64)
    cls, prob = argmax_prob(x, temperature)
    for b in range(B):
        void = (lab[b] == ignore) | (lab[b] < 0) | (lab[b] >= C)
        # iou_counts takes labels outside [0, C) as "no class": hand it the void rows as -1
        counts[b], _ = iou_counts(x[b], np.where(void, -1, lab[b]), C)
        np.add.at(conf, (np.where(void, C, lab[b]), cls[b]), 1)
        keep = np.flatnonzero(~void)
        if keep.size:
            r = ce_rows(x[b][keep], lab[b][keep], C, ignore)
            loss[b] = r["loss"] * r["count"], r["count"]
    return {"img_counts": counts, "confusion": conf, "img_loss": loss, "cls": cls, "prob": prob}


def _ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.zeros(np.broadcast(num, den).shape, np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


def image_iou(counts, smooth=1e-6):
    """compute_iou_for_image from one image's (I, P, L): classes with an empty union are skipped; no class at all gives 1.0"""
    I, P, L = np.asarray(counts, np.float64)
    U = P + L - I
    seen = U > 0
    return float(np.mean((I[seen] + smooth) / (U[seen] + smooth))) if seen.any() else 1.0


def batch_iou(counts, smooth=1e-6):
    """mean_iou of a batch from its per-image counts [B,3,C]; NaN if no class has a union"""
    I, P, L = np.asarray(counts, np.float64).sum(axis=0)
    U = P + L - I
    seen = U > 0
    return float(np.mean((I[seen] + smooth) / (U[seen] + smooth))) if seen.any() else float("nan")


def metrics(confusion, per_update_img_counts, per_update_img_loss, smooth=1e-6):
    """metrics_from_counts, restated: see the contract in maskunet_amd/metrics.py"""
    conf = np.asarray(confusion, np.int64)
    C = conf.shape[1]
    real = conf[:C]
    tp = np.array([real[c, c] for c in range(C)], np.int64)
    support = np.array([real[c].sum() for c in range(C)], np.int64)
    fp = np.array([real[:, c].sum() - real[c, c] for c in range(C)], np.int64)
    fn = support - tp
    present = (tp + fp + fn) > 0
    out = {"confusion": conf, "tp": tp, "fp": fp, "fn": fn, "support": support, "present": present,
           "iou": _ratio(tp, tp + fp + fn), "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn),
           "f1": _ratio(2 * tp, 2 * tp + fp + fn)}
    n = float(support.sum())
    for name, macro in (("iou", "miou"), ("precision", "macro_precision"), ("recall", "macro_recall"), ("f1", "macro_f1")):
        v = out[name]
        out[macro] = float(np.mean(v[present])) if present.any() else 0.0
        out["weighted_" + name] = float(np.sum(v * support) / n) if n else 0.0
    out["pixel_accuracy"] = float(tp.sum() / n) if n else 0.0
    out["mean_accuracy"] = float(np.mean(out["recall"][support > 0])) if (support > 0).any() else 0.0
    losses = []
    for ls in per_update_img_loss:
        ls = np.asarray(ls, np.float64)
        losses.append(ls[:, 0].sum() / ls[:, 1].sum() if ls[:, 1].sum() > 0 else float("nan"))
    out["reference"] = {
        "batch_miou": float(np.mean([batch_iou(c, smooth) for c in per_update_img_counts])),
        "image_miou": float(np.mean([image_iou(c, smooth) for cs in per_update_img_counts for c in cs])),
        "loss": float(np.mean(losses)),
    }
    return out
