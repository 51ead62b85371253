#!/usr/bin/env python3
"""Golden vectors for the embedding-instance post-processing (build container only; needs the reference checkout and sklearn, CPU).

get_instances_from_embeddings and get_instance_annotations are AST-extracted from city_instance.py at generation time (no reference
text is kept) and run with the installed sklearn's DBSCAN; pycocotools is not needed: mask_to_rle is stubbed to return the mask.
Stored per case: cls, emb, num_classes, eps, min_samples, the reference's instance map, its annotations (bbox, category_id, score) and
the margin min |d^2 - eps^2| / eps^2 over same-class pairs.  The margin is asserted > 1e-6, which keeps sklearn's own distance
arithmetic out of the result, and every case is asserted to exercise every rule of the contract (tests/_dbscan_reference.py)."""
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _dbscan_reference as R  # noqa: E402

REF = "/root/reference/code"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dbscan")     # a folder of its own: tests/golden/*.npz are the module cases
MIN_MARGIN = 1e-6

# name -> (seed, H, W, D, class sizes (class 1, 2, ...), dtype).  Seeds were picked so that the margin holds.
CASES = {
    "dbscan_16x16_d16": (11, 16, 16, 16, [60, 3, 45, 0, 30], np.float32),
    "dbscan_32x32_d16": (16, 32, 32, 16, [270, 4, 230, 300], np.float32),
    "dbscan_20x24_d3_fp16": (13, 20, 24, 3, [120, 2, 150], np.float16),
}


def load_functions(path, names):
    from sklearn.cluster import DBSCAN
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {"np": np, "DBSCAN": DBSCAN, "mask_to_rle": lambda m: m}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def main():
    get_instances, get_annotations = load_functions(os.path.join(REF, "cityscapes/city_instance.py"),
                                                    ["get_instances_from_embeddings", "get_instance_annotations"])
    os.makedirs(OUT, exist_ok=True)
    for name, (seed, H, W, D, sizes, dtype) in CASES.items():
        cls, emb = R.clustered_case(seed, H, W, D, sizes, dtype)
        nc = len(sizes) + 1
        m = R.margin(cls, emb, nc, 0.5)
        assert m > MIN_MARGIN, (name, m)
        cov = R.rule_coverage(cls, emb, nc, 0.5, 5)
        assert cov["noise"] and cov["small_class"] and cov["two_clusters"] and cov["shared_border"], (name, cov)
        ids = get_instances(cls.astype(np.int64), emb.astype(np.float32), eps=0.5, min_samples=5)
        ann = get_annotations(ids, cls.astype(np.int64))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), cls=cls, emb=emb, num_classes=np.array(nc), eps=np.array(0.5, np.float32),
                            min_samples=np.array(5), ids=ids.astype(np.int32), margin=np.array(m),
                            bbox=np.array([a["bbox"] for a in ann], np.float64).reshape(-1, 4),
                            category_id=np.array([a["category_id"] for a in ann], np.int32),
                            score=np.array([a["score"] for a in ann], np.float64))
        print(f"wrote {name}: {int(ids.max())} instances, margin {m:.2e}, coverage {cov}")


if __name__ == "__main__":
    main()
