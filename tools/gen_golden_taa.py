"""Writes tests/golden/taa_69x21.npz with the numpy restatement of sah_taa_resolve (tests/taa_ref.py): the inputs and the output for both
settings of SAH_TAA_HDR_WEIGHTS.

    python tools/gen_golden_taa.py

69 x 21 is one tile of the kernel (64 x 16) plus five pixels in each axis.  A frame of constant depth surrounds the image (columns < 8 and
>= 61, rows < 3 and >= 18): every tap ties there, the pixel keeps its own motion vector, and that is where the motion vectors with a known
landing point are planted — q exactly on 0, W and H, on texel centres, outside, at inf and at NaN.  The jitters are dyadic, so
dj = previous_jitter - jitter = (-0.5, 0.5) exactly.  tests/test_taa_cpu.py asserts that each planted case takes its branch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import taa_ref  # noqa: E402

WIDTH, HEIGHT = taa_ref.TILE[0] + 5, taa_ref.TILE[1] + 5
FIXTURE = os.path.join(ROOT, "tests", "golden", f"taa_{WIDTH}x{HEIGHT}.npz")
BLEND, JITTER, PREVIOUS_JITTER = 0.25, (0.25, -0.125), (-0.25, 0.375)
f16 = np.float16
# (x, y, mv.x, mv.y) inside the constant-depth frame; q = (x + 0.5 + mv.x - 0.5, y + 0.5 + mv.y + 0.5)
PLANTED_MV = [(3, 9, -3.0, 0.25),      # q.x == 0
              (66, 9, 3.0, -0.75),     # q.x == W
              (30, 1, 0.125, -2.0),    # q.y == 0
              (30, 19, -0.25, 1.0),    # q.y == H
              (5, 12, 1.5, -0.5),      # q = (6.5, 12.5): a texel centre, every weight but one is zero
              (64, 5, 0.0, 0.0),       # no motion: the half-texel of dj alone
              (2, 6, -100.0, 0.0),     # outside, left
              (65, 14, 0.0, 300.0),    # outside, below
              (4, 15, np.inf, 0.0), (63, 7, 0.0, -np.inf), (6, 10, np.nan, 0.0), (62, 11, 0.0, np.nan)]
# (x, y, channel, value): lit
PLANTED_LIT = [(20, 8, 0, np.inf), (21, 12, 1, -np.inf), (35, 6, 2, np.nan), (36, 14, 0, -0.0), (45, 10, 1, -0.0), (0, 0, 0, 65504.0), (68, 20, 2, np.nan),
               (50, 5, 0, 6e-8), (51, 15, 1, -65504.0)]
PLANTED_HISTORY = [(15, 10, 0, np.nan), (40, 7, 1, np.inf), (55, 13, 2, -np.inf), (25, 16, 0, 65504.0), (26, 16, 0, 65504.0), (1, 10, 1, np.nan)]
# (x, y, bits): depth, inside the frame's interior
PLANTED_DEPTH = [(18, 7, 0x7fc00000), (33, 11, 0x7f800000), (47, 9, 0xff800000), (52, 13, 0x80000000)]


def _frame_mask():
    yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH]
    return (xx < 8) | (xx >= 61) | (yy < 3) | (yy >= 18)


def inputs(seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH]
    smooth = (1.5 + np.sin(xx * 0.31) * np.cos(yy * 0.47))[..., None] * np.array([1.0, 0.8, 0.6, 1.0])
    lit = (smooth + g.normal(0, 0.15, (HEIGHT, WIDTH, 4))).astype(f16)
    history = (smooth * 1.05 + g.normal(0, 0.25, (HEIGHT, WIDTH, 4))).astype(f16)
    # a block of lit and of history across the fp16 range (any finite pattern, alpha any pattern at all)
    wild = g.integers(0, 1 << 16, (HEIGHT, WIDTH, 4), dtype=np.uint16)
    finite = (wild & 0x7c00) != 0x7c00
    lit_bits, hist_bits = lit.view(np.uint16), history.view(np.uint16)
    lit_bits[5:12, 24:34] = np.where(finite, wild, 0x3c00)[5:12, 24:34]
    hist_bits[9:16, 30:44] = np.where(finite, wild, 0x3c00)[::-1][9:16, 30:44]
    lit_bits[..., 3] = wild[..., 3]
    hist_bits[..., 3] = wild[::-1, ::-1, 0]
    for x, y, ch, v in PLANTED_LIT:
        lit[y, x, ch] = v
    for x, y, ch, v in PLANTED_HISTORY:
        history[y, x, ch] = v
    depth = g.random((HEIGHT, WIDTH), dtype=np.float32)
    depth[5:14, 36:50] = (np.floor(depth[5:14, 36:50] * 4) / 4 + 0.125).astype(np.float32)  # four levels: ties between neighbours
    depth[12:17, 10:22] = 0.0                                                                # sky
    depth[_frame_mask()] = 0.5
    bits = depth.view(np.uint32)
    for x, y, b in PLANTED_DEPTH:
        bits[y, x] = b
    mv = g.uniform(-1.5, 1.5, (HEIGHT, WIDTH, 2)).astype(f16)
    for x, y, mx, my in PLANTED_MV:
        mv[y, x] = (mx, my)
    return lit.view(np.uint16), depth, mv.view(np.uint16), history.view(np.uint16)


def generate(seed):
    lit, depth, mv, history = inputs(seed)
    out = {"seed": np.int64(seed), "lit": lit, "depth": depth, "motion_vectors": mv, "history": history, "blend": np.float32(BLEND),
           "jitter": np.array(JITTER, np.float32), "previous_jitter": np.array(PREVIOUS_JITTER, np.float32)}
    out["out_plain"] = taa_ref.resolve(lit, depth, mv, history, BLEND, JITTER, PREVIOUS_JITTER, 0)
    out["out_hdr"] = taa_ref.resolve(lit, depth, mv, history, BLEND, JITTER, PREVIOUS_JITTER, taa_ref.HDR_WEIGHTS)
    return out


if __name__ == "__main__":
    data = generate(69)
    np.savez_compressed(FIXTURE, **data)
    _, info = taa_ref.resolve_ex(data["lit"], data["depth"], data["motion_vectors"], data["history"], BLEND, JITTER, PREVIOUS_JITTER, 0)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; valid {int(info['valid'].sum())}, clamped {int(info['clamped'].sum())}, "
          f"lit taken {int(info['fallback'].sum())} of {WIDTH * HEIGHT}; plain != hdr at {int((data['out_plain'] != data['out_hdr']).any(-1).sum())}")
