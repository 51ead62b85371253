#!/usr/bin/env python3
"""Golden vectors for the id-map ground-truth instances (build container only; needs the reference checkout, CPU).

get_instance_annotations is AST-extracted from city_instance.py at generation time (no reference text is kept) and run on the cases of
tests/_idmap_reference.py; pycocotools is not needed: mask_to_rle is stubbed to return the mask.  The colour case goes through
panopticapi's published rgb2id first, as coco_panoptic.py does.  Stored per case: the inputs (id_map, sem) and, in the order in which
the reference appends its annotations, bbox, category_id, area (the mask's pixel count) and the masks as one id map (annotation k -> k + 1).
Every case is asserted to contain what it is named for."""
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _cc_reference as CC  # noqa: E402
from tests import _idmap_reference as R  # noqa: E402

REF = "/root/reference/code"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "idmap")     # a folder of its own: tests/golden/*.npz are the module cases


def load_function(path, name):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    ns = {"np": np, "mask_to_rle": lambda m: m}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def check_named_content(name, v, sem, ann):
    cats = [a["category_id"] for a in ann]
    if name == "idmap_cityscapes_32x32":
        vals = np.unique(v[v != 0])
        assert (vals < 1000).any() and (vals >= 1000).any(), "stuff and thing values"
        assert ((sem == 255) & (v >= 1000)).any(), "ignore label inside instances"
        assert 255 in cats and 26 in cats
        _, regions = CC.label_image((v == 26000).astype(np.int32))
        assert len(regions) == 2, "one instance in two pieces"
        _, regions = CC.label_image(((v == 26001) | (v == 26002)).astype(np.int32))
        assert len(regions) == 1 and (sem[v == 26001] != 255).any(), "two touching instances of one class"
    elif name == "idmap_negative_20x24":
        assert (v < 0).any()
        differ = 0
        for val in np.unique(v[v != 0]):
            c = np.sort(sem[v == val])
            if len(c) % 2 == 0 and c[len(c) // 2 - 1] != c[len(c) // 2]:
                differ += 1
        assert differ >= 2, "even areas whose two middle classes differ"
    else:
        assert (v > 65535).any() and (v[v != 0] < 65536).any()


def main():
    annotate = load_function(os.path.join(REF, "cityscapes/city_instance.py"), "get_instance_annotations")
    os.makedirs(OUT, exist_ok=True)
    for name, make in R.GOLDEN.items():
        id_map, sem = make()
        v = R.rgb2id(id_map[0]) if id_map.ndim == 4 else id_map[0]
        ann = annotate(v, sem[0])
        check_named_content(name, v, sem[0], ann)
        masks = np.zeros(v.shape, np.int32)
        for k, a in enumerate(ann):
            assert not masks[a["segmentation"] == 1].any()
            masks[a["segmentation"] == 1] = k + 1
        np.savez_compressed(os.path.join(OUT, name + ".npz"), id_map=id_map, sem=sem, masks=masks,
                            bbox=np.array([a["bbox"] for a in ann], np.float64).reshape(-1, 4),
                            category_id=np.array([a["category_id"] for a in ann], np.int32),
                            area=np.array([int(a["segmentation"].sum()) for a in ann], np.int32))
        print(f"wrote {name}: {len(ann)} annotations, categories {sorted(set(a['category_id'] for a in ann))}")


if __name__ == "__main__":
    main()
