"""Writes tests/golden/pil/pil_c{1,3}.npz: the bytes that the INSTALLED Pillow gives for Image.resize((Wd, Hd), Image.BILINEAR) on the
integer-formula inputs of tests/_pil_reference.pattern, plus Pillow's version string.  Only Pillow's outputs are stored; the inputs are
regenerated from the formula by every test.  Run from the repository root:  python tests/golden/make_golden_pil.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import _pil_reference as R  # noqa: E402


def main():
    import PIL
    from PIL import Image
    out_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pil")
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for c in (1, 3):
        arrays = {"pillow_version": np.array(PIL.__version__)}
        for h, w, cc, kind, Hd, Wd in R.fixture_cases():
            if cc != c:
                continue
            src = R.pattern(h, w, c, kind)
            got = np.asarray(Image.fromarray(src).resize((Wd, Hd), Image.BILINEAR))
            assert got.dtype == np.uint8 and got.shape[:2] == (Hd, Wd)
            arrays[R.fixture_key(h, w, c, kind, Hd, Wd)] = got
        path = os.path.join(out_dir, f"pil_c{c}.npz")
        np.savez_compressed(path, **arrays)
        total += os.path.getsize(path)
        print(path, len(arrays) - 1, "cases", os.path.getsize(path), "bytes")
    print("total", total, "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
