"""Writes tests/golden/lighting_vrs_75x45.npz with the numpy restatement of include/sah_vrs.h (tests/lighting_vrs_ref.py).

    python tools/gen_golden_vrs.py

75 x 45 with texels of 8 x 8 is the first parity case of the restatement: three 32 x 32 regions by two, the last ones 11 columns and 13 rows
wide, the last texels 3 columns and 5 rows, coarse pixels cut on both edges.  The fixture holds the case's depth plane and shading-rate
image, the source map at TOLERANCE, at +infinity and at 0, and a 2 x (37 x 21) frame of halfs — finite values of every magnitude, subnormals,
65504s, infinities of both signs, NaNs — with its resolve."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lighting_vrs_ref as ref  # noqa: E402

WIDTH, HEIGHT, TEXEL = ref.PARITY_CASES[0]
FIXTURE = os.path.join(ROOT, "tests", "golden", f"lighting_vrs_{WIDTH}x{HEIGHT}.npz")
RESOLVE_EXTENT = (37, 21)  # of the output
TOLERANCES = (ref.TOLERANCE, float("inf"), 0.0)


def resolve_input(w, h, seed):
    """(2h, 2w, 4) uint16: random halfs of every exponent, then blocks of special values"""
    g = np.random.default_rng(seed)
    lit = g.integers(0, 0x7c00, (2 * h, 2 * w, 4), dtype=np.uint16) | (g.integers(0, 2, (2 * h, 2 * w, 4), dtype=np.uint16) << 15)
    lit[0:2, 0:2] = 0x7bff                                   # 65504 four times: no overflow in fp32
    lit[0:2, 2:4] = 0x0001                                   # the smallest subnormal: the mean rounds to even, 0
    lit[0:2, 4:6, 0], lit[0, 4, 0] = 0x0001, 0x0003          # subnormals whose mean is a tie
    lit[2:4, 0:2] = 0x7c00                                   # +inf
    lit[2:4, 2:4], lit[2, 2] = 0x7c00, 0xfc00                # +inf and -inf: NaN
    lit[2:4, 4:6], lit[3, 5, 1] = 0x3c00, 0x7e01             # one NaN among ones, in one channel
    lit[4:6, 0:2], lit[4, 0] = 0x7bff, 0xfbff                # 65504 and -65504
    lit[-2:, -2:], lit[-1, -1, 3] = 0x0400, 0xfd00           # the last block: the smallest normal, a negative NaN in alpha
    return lit


def generate():
    depth, rates = ref.parity_inputs(0)
    maps = np.stack([np.stack(ref.source_map(depth, rates, TEXEL, t)) for t in TOLERANCES]).astype(np.int16)
    lit = resolve_input(*RESOLVE_EXTENT, 77)
    return {"depth": depth, "rate_image": rates, "texel_size": np.array(TEXEL, np.int64), "tolerances": np.array(TOLERANCES, np.float32),
            "source_map": maps, "resolve_in": lit, "resolve_out": ref.resolve(lit)}


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(FIXTURE, **data)
    sy, sx = data["source_map"][0]
    yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH]
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; {float(((sy != yy) | (sx != xx)).mean()):.2f} of the pixels take another pixel's value")
