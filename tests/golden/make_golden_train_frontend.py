"""Writes tests/golden/train_frontend_pil.npz: what Pillow itself gives on cases of tests/train_frontend_reference.py.
Outputs only - the sources are closed-form from seeds (train_frontend_reference.source).  Needs Pillow; run from the
repository root:  python tests/golden/make_golden_train_frontend.py

  <case>  Image.fromarray(a).crop(box).resize((RW, RH), Image.BICUBIC), the whole resized crop, for GOLDEN_CASES
  <eval>  Image.fromarray(a).resize((RW, RH), Image.BICUBIC).crop(centre window) with torchvision's Resize + CenterCrop
          geometry, for GOLDEN_EVAL
"""
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import train_frontend_reference as R  # noqa: E402


def main():
    out = {}
    for name in R.GOLDEN_CASES:
        _, (x0, y0, bw, bh), (RW, RH), _, _, _, _ = R.CASES[name]
        im = Image.fromarray(R.case_source(name)).crop((x0, y0, x0 + bw, y0 + bh)).resize((RW, RH), Image.BICUBIC)
        out[name] = np.asarray(im)
    for name, ((h, w), size) in R.GOLDEN_EVAL.items():
        RW, RH, ox, oy = R.eval_geometry(h, w, size)
        im = Image.fromarray(R.eval_source(name)).resize((RW, RH), Image.BICUBIC).crop((ox, oy, ox + size, oy + size))
        out[name] = np.asarray(im)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_frontend_pil.npz")
    np.savez_compressed(path, pillow_version=np.array(Image.__version__), **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
