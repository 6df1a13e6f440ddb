"""Writes the Pillow-encoded pictures of this directory and, beside each, the luma Pillow itself decodes from it (.luma.npy): real-encoder files
for tests/test_jpeg_cpu.py and tests/test_jpeg_gpu.py on machines without Pillow.  Run from the repository root: python tests/golden/jpeg/make_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
from tests import jpegref as J  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
# name: width, height, quality, optimised tables, Pillow's subsampling code (2: 4:2:0, 1: 4:2:2, 0: 4:4:4, None: grey), restart interval in MCUs
CASES = {"q50_420_72x40": (72, 40, 50, False, 2, 0), "q90opt_422_72x40": (72, 40, 90, True, 1, 0), "q90_444_40x24": (40, 24, 90, False, 0, 0),
         "q50opt_grey_40x24": (40, 24, 50, True, None, 0), "q90opt_420_64x48_dri": (64, 48, 90, True, 2, 3)}

for name, (w, h, q, opt, sub, dri) in CASES.items():
    y, u, v = J.picture(w, h, q + w)
    b = io.BytesIO()
    kw = dict(quality=q, optimize=opt)
    if dri:
        kw["restart_marker_blocks"] = dri
    if sub is None:
        Image.fromarray(y, "L").save(b, "JPEG", **kw)
    else:
        Image.fromarray(np.stack([y, u, v], axis=-1), "YCbCr").save(b, "JPEG", subsampling=sub, **kw)
    data = b.getvalue()
    assert len(data) <= 8192, (name, len(data))
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    im.load()
    luma = np.asarray(im) if im.mode == "L" else np.asarray(im)[..., 0]
    open(os.path.join(HERE, name + ".jpg"), "wb").write(data)
    np.save(os.path.join(HERE, name + ".luma.npy"), np.ascontiguousarray(luma))
    print(name, len(data), "bytes")
