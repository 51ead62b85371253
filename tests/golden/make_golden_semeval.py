#!/usr/bin/env python3
"""Golden vectors for the semantic evaluation (build container only; needs /root/reference, CPU).

compute_iou_for_image and mean_iou are AST-extracted from cityscapes/city_panoptic.py (:212-236) at generation time and run on small
inputs the way the validation loops call them: mean_iou(outputs, labels, c_out) on the batch, and per image
compute_iou_for_image(pred_mask, gt_mask, c_out) with preds = argmax(softmax(outputs / 0.5)) (evaluate_panoptic_metrics).
Stored per case: y (logits, fp16-exact values), t (labels, 255 = the ignore label of the Cityscapes scripts), num_classes,
image_iou [B], image_miou (their mean), splits (the batch sizes of consecutive updates) and batch_miou [len(splits)].
"""
import ast
import os

import numpy as np
import torch

REF = "/root/reference/code"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "semeval")     # tests/golden/*.npz itself is globbed as module cases


def load_functions(path, names):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def case(name, fns, B, C, H, W, seed, splits, void_image=None, label_hi=None, p_ignore=0.1):
    image_fn, batch_fn = fns
    rng = np.random.default_rng(seed)
    # a 1/8 grid after a ReLU: exact in fp16, and ties between maxima are common (the first one must win)
    y = np.maximum(rng.integers(-24, 41, (B, C, H, W)) / 8.0, 0.0).astype(np.float16)
    t = rng.integers(0, C if label_hi is None else label_hi, (B, H, W)).astype(np.int64)
    t[rng.random((B, H, W)) < p_ignore] = 255
    t[0, 0, 0], t[0, 0, 1] = 0, C - 1
    if void_image is not None:
        t[void_image] = 255
    yt, tt = torch.from_numpy(y.astype(np.float32)), torch.from_numpy(t)
    preds = torch.argmax(torch.softmax(yt / 0.5, dim=1), dim=1).numpy()
    image_iou = np.array([float(image_fn(preds[b], t[b], C)) for b in range(B)], np.float64)
    assert sum(splits) == B
    edges = np.cumsum([0] + list(splits))
    batch = np.array([float(batch_fn(yt[a:b], tt[a:b], C)) for a, b in zip(edges[:-1], edges[1:])], np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), y=y, t=t.astype(np.int16), num_classes=np.array(C), image_iou=image_iou,
                        image_miou=np.array(image_iou.mean()), splits=np.array(splits), batch_miou=batch)
    print("wrote", name, "image_miou", image_iou.mean(), "batch_miou", batch)


def main():
    fns = load_functions(os.path.join(REF, "cityscapes/city_panoptic.py"), ["compute_iou_for_image", "mean_iou"])
    case("semeval_city19", fns, 3, 19, 12, 10, 701, [3])
    case("semeval_void_image", fns, 3, 19, 12, 10, 702, [3], void_image=1)                 # image 1: every pixel is void
    case("semeval_absent_classes", fns, 2, 21, 8, 8, 703, [1, 1], label_hi=15)             # classes 15..20 never labelled
    case("semeval_updates_19", fns, 6, 19, 24, 20, 704, [1, 2, 3])                          # the three updates of the GPU test


if __name__ == "__main__":
    main()
