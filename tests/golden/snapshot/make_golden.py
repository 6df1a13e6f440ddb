"""Writes the fixtures of tests/test_snapshot_cpu.py: grey JPEGs made by Pillow (libjpeg-turbo, its accurate integer forward DCT) of small planes, and the planes.
The pin of section 18's arithmetic to libjpeg then holds where Pillow is absent.  Run from the repository root: python tests/golden/snapshot/make_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
from tests import snapref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
# (name, width, height, content, quality, tables: "luma" = Pillow's own of that quality, "chroma" = the chroma table through qtables=)
CASES = [("textured_72x40_q75", 72, 40, "textured", 75, "luma"), ("noise_64x40_q50", 64, 40, "noise", 50, "luma"), ("saturated_41x23_q100", 41, 23, "saturated", 100, "luma"),
         ("noise_41x23_q10", 41, 23, "noise", 10, "luma"), ("textured_56x40_q90_chroma", 56, 40, "textured", 90, "chroma")]


def plane(w, h, kind):
    y, _ = snapref.picture((w + 1) & ~1, (h + 1) & ~1, kind, seed=2)
    return np.ascontiguousarray(y[:h, :w])


def grey_jpeg(p, quality, tables):
    buf = io.BytesIO()
    if tables == "chroma":
        Image.fromarray(p, "L").save(buf, "JPEG", qtables=[[int(v) for v in snapref.tables(quality)[1]]])  # (qtables= takes the 64 values in natural order)
    else:
        Image.fromarray(p, "L").save(buf, "JPEG", quality=quality)
    return buf.getvalue()


if __name__ == "__main__":
    for name, w, h, kind, q, tables in CASES:
        p = plane(w, h, kind)
        np.save(os.path.join(HERE, name + ".plane.npy"), p)
        with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
            f.write(grey_jpeg(p, q, tables))
