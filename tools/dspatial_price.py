"""What the spatial noise filter buys and costs, beside the temporal filter's rows of tools/denoise_price.py on the same clip.

The benchmark's clip (synth.s2_frames, 1080p: a pan with moving objects) plus seeded Gaussian noise of sigma 3 on every plane, coded IPPP at fixed QP 26 / 32 / 38
with the step off, manual at strength 6 (luma = chroma), automatic (twice the measured sigma, bounds 32) -- and, for comparison, the temporal filter alone at
strength 4 and 8 and the spatial filter in front of the temporal one.  Per case, over the P pictures: bytes per picture, PSNR-Y of the source surfaces (what
the encoder codes) against the CLEAN clip, PSNR-Y of the reconstruction against the clean clip, and in automatic mode the strengths the pictures were filtered
with.  Prints a markdown table and writes it to profiles/dspatial_price.md."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ceracoder_amd import enc as E  # noqa: E402
from ceracoder_amd import synth  # noqa: E402
from tools.denoise_price import H, SIGMA, W, clips  # noqa: E402

CASES = (("off", None, None), ("spatial, manual 6", dict(luma=6, chroma=6), None), ("spatial, automatic (gain 2, bounds 32)", dict(luma=32, chroma=32, auto_gain=2000), None),
         ("temporal 4", None, dict(luma=4, chroma=4)), ("temporal 8", None, dict(luma=8, chroma=8)),
         ("spatial automatic, then temporal 4", dict(luma=32, chroma=32, auto_gain=2000), dict(luma=4, chroma=4)))


def price(n):
    clean, noisy = clips(n, False)
    out = ["The benchmark's clip (a pan with moving objects), 1080p, %d pictures, Gaussian noise sigma %g; means over the P pictures.\n" % (n, SIGMA),
           "| QP | filter | bytes / P picture | PSNR-Y of the source against the clean clip (dB) | PSNR-Y of the reconstruction against the clean clip (dB) | strengths (luma) |",
           "|---|---|---|---|---|---|"]
    for line in out:
        print(line, flush=True)
    for qp in (26, 32, 38):
        for name, ds, dn in CASES:
            e = E.Encoder(W, H, fps=60, gop=n, fixed_qp=qp, denoise_spatial=ds, denoise=dn)
            size, psnr, src, ss = [], [], [], set()
            for i in range(n):
                au = e.encode(*noisy[i], pts=i)[0]
                ss.add(e.last_denoise_spatial()[1]["s_luma"])
                if i == 0:
                    continue
                size.append(len(au))
                psnr.append(synth.psnr(e.fetch(E.FETCH_RECON_Y)[:H, :W], clean[i][0]))
                src.append(synth.psnr(e.fetch(E.FETCH_SOURCE_Y)[:H, :W], clean[i][0]))
            e.close()
            out.append("| %d | %s | %d | %.2f | %.2f | %s |" % (qp, name, round(np.mean(size)), np.mean(src), np.mean(psnr), " ".join(str(s) for s in sorted(ss)) if ds else "-"))
            print(out[-1], flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dspatial_price.md"), "w") as f:
        f.write("# The spatial noise filter's price (tools/dspatial_price.py; DESIGN.md section 30)\n\n" + "\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=12)
    price(ap.parse_args().pictures)
