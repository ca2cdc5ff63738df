"""Writes tests/golden/vrsaa_97x61.npz with the numpy restatement of the two VRSAA passes (tests/vrsaa_ref.py): inputs, the contrast
image and the 13 x 8 shading-rate image (an 8 x 8 texel size) for the seven rates of vrsaa_ref.RATES.

    python tools/gen_golden_vrsaa.py

Width 97 and height 61 are extents at which the sampler's index lands one texel low for some columns and rows (vrsaa_ref.low_landing).
Colour is random bytes.  Depth is mostly uniform in [0, 1); +inf, -inf, NaN, -0 and a denormal are planted away from each other, one of
them on a low-landing column and one on the border; a few smooth patches keep some texels under the saturation of the rate search."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import vrsaa_ref  # noqa: E402

WIDTH, HEIGHT, TEXEL = 97, 61, 8
SRI_EXTENT = (13, 8)  # ceil(97 / 8), ceil(61 / 8)
FIXTURE = os.path.join(ROOT, "tests", "golden", "vrsaa_97x61.npz")
# (x, y, bits): x = 13 is a low-landing column of width 97, (0, 30) and (96, 60) lie on the border
PLANTED = [(13, 20, 0x7f800000), (0, 30, 0xff800000), (50, 10, 0x7fc00000), (70, 40, 0x80000000), (30, 50, 0x00000123), (96, 60, 0x7f800000)]


def inputs(seed):
    g = np.random.default_rng(seed)
    color = g.integers(0, 256, (HEIGHT, WIDTH, 4), dtype=np.uint8)
    depth = g.random((HEIGHT, WIDTH), dtype=np.float32)
    # flat patches (equal colour, equal depth): zero gradients inside, so that the shading-rate image holds more than one code
    # and ramps (depth falling by sy per row and sx per column: Sobel sums of 8 * sy and 8 * sx, under the search's saturation at 0.8)
    for (x0, y0, x1, y1, sx, sy) in ((0, 0, 30, 18, 0.0, 0.0), (40, 24, 97, 44, 0.02, 0.05), (56, 0, 80, 9, 0.07, 0.02)):
        color[y0:y1, x0:x1] = color[y0, x0]
        yy, xx = np.mgrid[0:y1 - y0, 0:x1 - x0]
        depth[y0:y1, x0:x1] = (0.95 - sy * yy - sx * xx).astype(np.float32)
    bits = depth.view(np.uint32)
    for x, y, b in PLANTED:
        bits[y, x] = b
    return color, depth


def generate(seed):
    color, depth = inputs(seed)
    contrast = vrsaa_ref.contrast(color, depth)
    sri = vrsaa_ref.shading_rate_image(contrast, SRI_EXTENT, vrsaa_ref.RATES)
    return {"seed": np.int64(seed), "color": color, "depth": depth, "contrast": contrast, "shading_rate_image": sri,
            "rates": np.array(vrsaa_ref.RATES, np.uint32)}


if __name__ == "__main__":
    out = generate(97)
    np.savez_compressed(FIXTURE, **out)
    codes, counts = np.unique(out["shading_rate_image"], return_counts=True)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; codes {dict(zip(codes.tolist(), counts.tolist()))}; "
          f"+inf texels {int((out['contrast'] == 0x7c00).sum())}")
