"""Writes tests/golden/taa_upscale_89x23_to_133x35.npz with the numpy restatement of sah_taa_upscale (tests/taa_upscale_ref.py): the inputs
and the output for both settings of SAH_TAA_HDR_WEIGHTS and without a history.

    python tools/gen_golden_taa_upscale.py

89 x 23 to 133 x 35: ratios of 1.494 and 1.522, neither an integer, and 3 x 3 tiles of the kernel (64 x 16) in the output, the last column
of tiles five pixels wide and the last row three high.  As in the TAA fixture a frame of constant depth surrounds the render image (columns
< 8 and >= 81, rows < 3 and >= 20): every tap ties there, the texel keeps its own motion vector, and that is where the motion vectors with
a known fate are planted — outside, at inf, at NaN, none at all.  The ratios are not dyadic, so no position is planted exactly on 0, W or
H.  tests/test_taa_upscale_cpu.py asserts that each planted case takes its branch and that every branch of Store has pixels."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import taa_upscale_ref as ref  # noqa: E402

RENDER, OUTPUT = (89, 23), (133, 35)
FIXTURE = os.path.join(ROOT, "tests", "golden", f"taa_upscale_{RENDER[0]}x{RENDER[1]}_to_{OUTPUT[0]}x{OUTPUT[1]}.npz")
BLEND, MIN_CONFIDENCE, JITTER, PREVIOUS_JITTER = 0.25, 0.05, (0.25, -0.125), (-0.25, 0.375)
f16 = np.float16
# (x, y, mv.x, mv.y) at render texels inside the constant-depth frame
PLANTED_MV = [(84, 5, 0.0, 0.0),       # no motion: dj alone, three quarters of an output pixel
              (5, 12, 1.5, -0.5),
              (3, 9, -100.0, 0.0),     # outside, left
              (85, 14, 0.0, 300.0),    # outside, below
              (4, 15, np.inf, 0.0), (84, 7, 0.0, -np.inf), (6, 10, np.nan, 0.0), (83, 11, 0.0, np.nan)]
# (x, y, channel, value): lit (render texels)
PLANTED_LIT = [(20, 8, 0, np.inf), (21, 12, 1, -np.inf), (35, 6, 2, np.nan), (36, 14, 0, -0.0), (45, 10, 1, -0.0), (0, 0, 0, 65504.0), (88, 22, 2, np.nan),
               (50, 5, 0, 6e-8), (51, 15, 1, -65504.0)]
# (X, Y, channel, value): history (output pixels)
PLANTED_HISTORY = [(15, 10, 0, np.nan), (60, 7, 1, np.inf), (100, 20, 2, -np.inf), (25, 30, 0, 65504.0), (26, 30, 0, 65504.0), (1, 10, 1, np.nan)]
# (x, y, bits): depth, inside the frame's interior
PLANTED_DEPTH = [(18, 7, 0x7fc00000), (33, 11, 0x7f800000), (47, 9, 0xff800000), (52, 13, 0x80000000)]


def _frame_mask():
    yy, xx = np.mgrid[0:RENDER[1], 0:RENDER[0]]
    return (xx < 8) | (xx >= 81) | (yy < 3) | (yy >= 20)


def _image(g, w, h, gain, noise):
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = (1.5 + np.sin(xx * (27.6 / w)) * np.cos(yy * (10.8 / h)))[..., None] * np.array([1.0, 0.8, 0.6, 1.0])
    return (smooth * gain + g.normal(0, noise, (h, w, 4))).astype(f16)


def inputs(seed):
    g = np.random.default_rng(seed)
    (w, h), (W, H) = RENDER, OUTPUT
    lit, history = _image(g, w, h, 1.0, 0.15), _image(g, W, H, 1.05, 0.25)
    # a block of lit and of history across the fp16 range (any finite pattern, alpha any pattern at all)
    lit_bits, hist_bits = lit.view(np.uint16), history.view(np.uint16)
    for bits, (ys, xs) in ((lit_bits, (slice(5, 12), slice(24, 34))), (hist_bits, (slice(14, 24), slice(45, 66)))):
        wild = g.integers(0, 1 << 16, bits.shape, dtype=np.uint16)
        bits[ys, xs] = np.where((wild & 0x7c00) != 0x7c00, wild, 0x3c00)[ys, xs]
        bits[..., 3] = wild[..., 3]
    for x, y, ch, v in PLANTED_LIT:
        lit[y, x, ch] = v
    for x, y, ch, v in PLANTED_HISTORY:
        history[y, x, ch] = v
    depth = g.random((h, w), dtype=np.float32)
    depth[5:14, 36:50] = (np.floor(depth[5:14, 36:50] * 4) / 4 + 0.125).astype(np.float32)  # four levels: ties between neighbours
    depth[12:17, 10:22] = 0.0                                                                # sky
    depth[_frame_mask()] = 0.5
    bits = depth.view(np.uint32)
    for x, y, b in PLANTED_DEPTH:
        bits[y, x] = b
    mv = g.uniform(-1.5, 1.5, (h, w, 2)).astype(f16)
    for x, y, mx, my in PLANTED_MV:
        mv[y, x] = (mx, my)
    return lit.view(np.uint16), depth, mv.view(np.uint16), history.view(np.uint16)


def generate(seed):
    lit, depth, mv, history = inputs(seed)
    out = {"seed": np.int64(seed), "lit": lit, "depth": depth, "motion_vectors": mv, "history": history, "blend": np.float32(BLEND),
           "min_confidence": np.float32(MIN_CONFIDENCE), "jitter": np.array(JITTER, np.float32), "previous_jitter": np.array(PREVIOUS_JITTER, np.float32)}
    for key, flags in (("out_plain", 0), ("out_hdr", ref.HDR_WEIGHTS), ("out_no_history", ref.HISTORY_INVALID)):
        out[key] = ref.upscale(lit, depth, mv, history, OUTPUT, BLEND, MIN_CONFIDENCE, JITTER, PREVIOUS_JITTER, flags)
    return out


if __name__ == "__main__":
    data = generate(89)
    np.savez_compressed(FIXTURE, **data)
    _, info = ref.upscale_ex(data["lit"], data["depth"], data["motion_vectors"], data["history"], OUTPUT, BLEND, MIN_CONFIDENCE, JITTER, PREVIOUS_JITTER, 0)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; valid {int(info['valid'].sum())}, clamped {int(info['clamped'].sum())}, blended "
          f"{int((~info['fallback']).sum())}, upsampled {int(info['used_bilinear'].sum())}, nearest {int(info['used_nearest'].sum())} of "
          f"{OUTPUT[0] * OUTPUT[1]}; plain != hdr at {int((data['out_plain'] != data['out_hdr']).any(-1).sum())}")
