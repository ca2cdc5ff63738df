"""Writes tests/golden/rt_denoise_69x21.npz with the numpy restatement of sah_rt_denoise (tests/rt_denoise_ref.py): three frames' inputs,
and each frame's accum_out, length_out and `denoised` for passes 0 to 3.

    python tools/gen_golden_rt_denoise.py

69 x 21 is one tile of the temporal kernel (64 x 16) plus five pixels in each axis, and two tiles of the filter kernel (32 x 16) plus five and
one plus five.  Three bands of columns: near (z about 2), middle (z about 5) and far (z about 30): the steps between them take the
filter's depth weight to 0.  A block of sky in the middle band; a crease at column 35,
the normals on its two sides at a right angle; NaN and negative depths, zero and NaN normals and NaN samples at fixed places.
Frame 0 has no history (SAH_RT_DENOISE_HISTORY_INVALID).  Frame 1: a static camera under another jitter, so most pixels reproject onto
their own texel; a NaN planted in three history texels and a length of 0 in three; a block of sub-pixel motion (four taps) across the
edge of an occluder that covered a block last frame (some taps fail the depth test, others pass); motion that leaves the image at the left
and at the bottom (q outside, and taps outside).  Frame 2: last_frame_view is 0.5 further back (a dolly) while only the middle band's
previous depth agrees with that — the near band's history fails the depth test, the far band's passes it within depth_tolerance.  Each
frame's history is the frame before's accum_out and length_out.  tests/test_rt_denoise_cpu.py asserts that each planted case takes its
branch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import rt_denoise_ref as ref  # noqa: E402

WIDTH, HEIGHT, FRAMES = ref.TEMPORAL_TILE[0] + 5, ref.TEMPORAL_TILE[1] + 5, 3
FIXTURE = os.path.join(ROOT, "tests", "golden", f"rt_denoise_{WIDTH}x{HEIGHT}.npz")
f32 = np.float32
PARAMS = dict(max_history=32.0, depth_tolerance=0.1, depth_sharpness=50.0, normal_squarings=5)
PROJECTION = dict(p00=1.0, p11=2.0, p20=0.01, p21=-0.02, z_near=0.05)
JITTERS = [(0.25, -0.125), (-0.375, 0.25), (0.125, 0.375)]  # dyadic: a static camera's q is the pixel centre exactly
DOLLY = 0.5
SKY = (slice(6, 15), slice(26, 33))
CREASE = 35
OCCLUDER = (slice(10, 16), slice(44, 53))       # last frame (of frame 1) something nearer covered these texels
SUBPIXEL = (slice(8, 13), slice(40, 57))        # frame 1: motion of (0.5, 0.25) on top of the jitter's
LEAVES_LEFT = (slice(0, HEIGHT), slice(0, 4))   # frame 1: 6 pixels to the left
LEAVES_BOTTOM = (slice(15, HEIGHT), slice(10, 21))  # frame 1: 4.25 pixels down
NAN_DEPTH = [(3, 3), (20, 10), (50, 9)]
NEGATIVE_DEPTH = [(8, 7), (43, 18), (64, 12)]
ZERO_NORMAL = [(2, 9), (25, 12), (66, 6)]
NAN_NORMAL = [(6, 2), (45, 13), (62, 18)]
NAN_SAMPLE = [(5, 5), (22, 14), (48, 4), (60, 17)]
NAN_HISTORY = [(7, 11), (38, 4), (58, 16)]
ZERO_LENGTH = [(9, 12), (39, 5), (59, 17)]

_c, _s = np.cos(0.3), np.sin(0.3)
VIEW = np.array([[_c, 0.0, _s, 0.25], [0.0, 1.0, 0.0, -1.0], [-_s, 0.0, _c, 0.5], [0.0, 0.0, 0.0, 1.0]])  # [row][column]: a turn about y, a shift


def view(frame):
    last = VIEW.copy()
    if frame == 2:
        last[2, 3] -= DOLLY  # last frame's camera stood DOLLY further back: z_prev = z + DOLLY
    return ref.View.of(inverse_view=np.linalg.inv(VIEW), last_frame_view=last, **PROJECTION)


def params(frame, passes):
    return dict(PARAMS, passes=passes, jitter=JITTERS[frame], previous_jitter=JITTERS[max(frame - 1, 0)], flags=0 if frame else ref.HISTORY_INVALID)


def scene(seed):
    """depth, normals (uint16 bits) and linear depth of the static scene"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH]
    bumps = np.sin(xx * 0.9) * np.cos(yy * 0.7)
    z = np.where(xx < 24, 2.0 + 0.01 * bumps, np.where(xx < 46, 5.0 + 0.05 * bumps, 30.0 + 0.2 * bumps))
    depth = (PROJECTION["z_near"] / z).astype(f32)
    depth[SKY] = 0.0
    for x, y in NAN_DEPTH:
        depth[y, x] = np.nan
    for x, y in NEGATIVE_DEPTH:
        depth[y, x] = -0.25
    n = np.zeros((HEIGHT, WIDTH, 4))
    n[:, :CREASE, 2], n[:, CREASE:, 0] = 1.0, 1.0
    n[..., :3] += g.normal(0, 0.02, (HEIGHT, WIDTH, 3))
    n[..., :3] *= g.uniform(0.5, 2.0, (HEIGHT, WIDTH, 1))
    normals = n.astype(np.float16)
    for x, y in ZERO_NORMAL:
        normals[y, x, :3] = 0.0
    for i, (x, y) in enumerate(NAN_NORMAL):
        normals[y, x, i % 3] = np.nan
    return depth, normals.view(np.uint16), z


def frame_inputs(frame, seed, depth, z):
    """noisy, motion_vectors (uint16 bits) and previous_depth of one frame"""
    g = np.random.default_rng(seed + 100 * frame)
    noisy = (g.random((HEIGHT, WIDTH)) < 0.25 + 0.5 * (np.mgrid[0:HEIGHT, 0:WIDTH][1] / WIDTH)).astype(f32)  # the mean rises from left to right
    for x, y in NAN_SAMPLE:
        noisy[y, x] = np.nan
    mv = np.zeros((HEIGHT, WIDTH, 2))
    mv[...] = np.array(JITTERS[frame]) - np.array(JITTERS[max(frame - 1, 0)])
    previous_depth = depth.copy()
    if frame == 1:
        mv[SUBPIXEL] += (0.5, 0.25)
        mv[LEAVES_LEFT] += (-6.0, 0.0)
        mv[LEAVES_BOTTOM] += (0.0, 4.25)
        previous_depth[OCCLUDER] = f32(PROJECTION["z_near"] / 1.0)
    if frame == 2:
        mv[2:7, 50:60] += (0.25, -0.5)
        middle = (np.mgrid[0:HEIGHT, 0:WIDTH][1] >= 24) & (np.mgrid[0:HEIGHT, 0:WIDTH][1] < 46) & (depth > 0)
        previous_depth = np.where(middle, (PROJECTION["z_near"] / (z + DOLLY)).astype(f32), depth).astype(f32)
    return noisy, mv.astype(np.float16).view(np.uint16), previous_depth


def generate(seed):
    depth, normals, z = scene(seed)
    out = {"seed": np.int64(seed), "depth": depth, "normals": normals}
    history, history_length = None, None
    for frame in range(FRAMES):
        noisy, mv, previous_depth = frame_inputs(frame, seed, depth, z)
        if frame == 1:
            history, history_length = history.copy(), history_length.copy()
            for x, y in NAN_HISTORY:
                history[y, x] = np.nan
            for x, y in ZERO_LENGTH:
                history_length[y, x] = 0
        out[f"noisy{frame}"], out[f"motion_vectors{frame}"] = noisy, mv
        if frame:
            out[f"previous_depth{frame}"], out[f"history{frame}"], out[f"history_length{frame}"] = previous_depth, history, history_length.view(np.uint16)
        for passes in range(4):
            accum, length, denoised = ref.denoise(noisy, depth, normals, mv, previous_depth if frame else None, history, history_length, view(frame),
                                                  params(frame, passes))
            out[f"denoised{frame}_passes{passes}"] = denoised
        out[f"accum{frame}"], out[f"length{frame}"] = accum, length.view(np.uint16)
        history, history_length = accum, length
    return out


def frame_of(fx, frame):
    """the seven input planes of `frame` from a loaded (or generated) fixture; the previous-frame planes are None for frame 0"""
    get = lambda k: fx[k] if k in fx else None  # noqa: E731
    return dict(noisy=fx[f"noisy{frame}"], depth=fx["depth"], normals=fx["normals"], motion_vectors=fx[f"motion_vectors{frame}"],
                previous_depth=get(f"previous_depth{frame}"), history=get(f"history{frame}"), history_length=get(f"history_length{frame}"))


if __name__ == "__main__":
    data = generate(69)
    np.savez_compressed(FIXTURE, **data)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; lengths of frame 2: " + str(np.unique(data["length2"].view(np.float16), return_counts=True)))
