"""Writes tests/golden/sharpen_69x21.npz with the numpy restatement of sah_sharpen (tests/sharpen_ref.py).

    python tools/gen_golden_sharpen.py

69 x 21 is a multiple of neither dimension of the kernel's 64 x 16 tile, and odd: two tiles by two, the second ones five columns and five
rows wide, every row ending on a thread with one pixel.  The scene is stored with the padded pitch it was generated with (70 texels), the
padding holding a pattern no texel has.  It is the blocky image of sharpen_ref.blocky_inputs with a handful of unclean texels (NaN, +-inf,
a negative) and a clean -0, two of them moved onto the tile seam.  CASES names the calls: SAH_SHARPEN_DENOISE off and on, a NULL exposure
and a device exposure of 0.375, sharpness 1 and 0.5, pre_scale 1 and 0.25."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import sharpen_ref as ref  # noqa: E402

WIDTH, HEIGHT = 69, 21
PITCH = 70  # in texels
FIXTURE = os.path.join(ROOT, "tests", "golden", f"sharpen_{WIDTH}x{HEIGHT}.npz")
EXPOSURE = 0.375
# (exposure, settings)
CASES = [(None, dict(sharpness=1.0, pre_scale=1.0, flags=0)),
         (None, dict(sharpness=1.0, pre_scale=1.0, flags=ref.DENOISE)),
         (EXPOSURE, dict(sharpness=1.0, pre_scale=1.0, flags=0)),
         (EXPOSURE, dict(sharpness=0.5, pre_scale=0.25, flags=ref.DENOISE))]


def scene_of(seed):
    scene = ref.blocky_inputs(WIDTH, HEIGHT, seed, unclean=8)
    scene[15, 63, :3] = np.array([np.nan, 0.5, 0.25], np.float16).view(np.uint16)   # the last column of the first tile, its last row
    scene[16, 64, :3] = np.array([0.5, -2.0, 0.25], np.float16).view(np.uint16)     # the first column and row of the tile diagonally across
    return scene


def generate(seed):
    scene = scene_of(seed)
    plane = np.full((HEIGHT, PITCH, 4), np.uint16(0xA5A5))
    plane[:, :WIDTH] = scene
    outs = np.stack([ref.sharpen(scene, e, s) for e, s in CASES])
    return {"seed": np.int64(seed), "width": np.int64(WIDTH), "scene_plane": plane, "exposure": np.float32(EXPOSURE), "sharpened": outs}


if __name__ == "__main__":
    data = generate(6922)
    np.savez_compressed(FIXTURE, **data)
    ok = ref.eligible(data["scene_plane"][:, :WIDTH])
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; {int((~ok).sum())} pixels pass through")
