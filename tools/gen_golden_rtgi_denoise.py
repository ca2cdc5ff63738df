"""Writes tests/golden/rtgi_denoise_69x21.npz with the numpy restatement of sah_rtgi_denoise (tests/rtgi_denoise_ref.py): three frames'
inputs, each frame's accum_out and moments_out (once, they do not depend on the pass count) and its denoised irradiance for passes 0 to 3.

    python tools/gen_golden_rtgi_denoise.py

69 x 21 is one tile of the temporal kernel (64 x 8) plus five pixels across and two plus five down, and four tiles of the filter kernel
(16 x 16) plus five and one plus five.  The surfaces, the views, the jitters, the motion vectors and the previous depths are those of
tools/gen_golden_rt_denoise.py (three depth bands, a crease, sky, NaN and negative depths, zero and NaN normals; frame 0 without a history,
frame 1 a static camera under another jitter with sub-pixel motion, an occluder and motion that leaves the image, frame 2 a dolly), with
a second block of sky so that the file stays small.  On top: one ray per pixel from a set of 32 directions and 8 distances, an irradiance
that is 0 for 70 % of the pixels and otherwise one of 8 levels — a quarter as bright left of column 12, an irradiance edge on the flat
near band — with inf and NaN components at fixed places; frame 1's history has a NaN colour in three texels, a sample count of 0 in three
and an inf moment in three.  min_history is 2, so that frames 1 and 2 have pixels on both sides of it.  Each frame's history is the frame
before's accum_out and moments_out; the fixture stores what differs from that (frame 1's planted texels are applied by frame_of).
tests/test_rtgi_denoise_cpu.py asserts that each planted case takes its branch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_rt_denoise as base  # noqa: E402
from tests import rtgi_denoise_ref as ref  # noqa: E402

WIDTH, HEIGHT, FRAMES = base.WIDTH, base.HEIGHT, 3
FIXTURE = os.path.join(ROOT, "tests", "golden", f"rtgi_denoise_{WIDTH}x{HEIGHT}.npz")
f32 = np.float32
PARAMS = dict(max_history=32.0, min_history=2.0, depth_tolerance=0.1, depth_sharpness=50.0, normal_squarings=5, luminance_sigma=4.0, luminance_floor=1e-6)
SKY2 = (slice(0, 7), slice(36, WIDTH))  # a second block of sky
EDGE = 12                               # the irradiance edge on the near band
NONFINITE_IRRADIANCE = [(5, 9, np.nan), (22, 14, np.inf), (48, 10, np.nan), (60, 17, -np.inf)]  # (x, y, value)
NAN_HISTORY = [(7, 11), (38, 9), (58, 16)]
ZERO_COUNT = [(9, 12), (39, 10), (59, 17)]
INF_MOMENT = [(11, 13), (41, 11), (61, 18)]
view = base.view


def params(frame, passes):
    return dict(PARAMS, passes=passes, jitter=base.JITTERS[frame], previous_jitter=base.JITTERS[max(frame - 1, 0)], flags=0 if frame else ref.HISTORY_INVALID)


def scene(seed):
    depth, normals, z = base.scene(seed)
    depth[SKY2] = 0.0
    return depth, normals, z


def frame_inputs(frame, seed, depth, z):
    """ray_buffer, ray_irradiance, motion_vectors (uint16 bits) and previous_depth of one frame"""
    _, mv, previous_depth = base.frame_inputs(frame, seed, depth, z)
    previous_depth = np.where(depth == 0, depth, previous_depth).astype(f32)
    g = np.random.default_rng(seed + 1000 * (frame + 1))
    dirs = g.normal(0, 1.0, (32, 3))
    dirs[:, 2] = np.abs(dirs[:, 2]) + 0.3
    dirs[16:, 0] = np.abs(dirs[16:, 0]) + 0.3  # (the normals right of the crease point along x)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    xx = np.mgrid[0:HEIGHT, 0:WIDTH][1]
    pick = g.integers(0, 16, (HEIGHT, WIDTH)) + 16 * (xx >= base.CREASE)
    rays = np.concatenate([dirs[pick], g.choice(np.array([0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 100.0]), (HEIGHT, WIDTH, 1))], -1).astype(np.float16)
    levels = np.array([0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]) * 0.0031415927 * 8.0
    hit = g.random((HEIGHT, WIDTH)) < 0.3
    irr = (hit * g.choice(levels, (HEIGHT, WIDTH)) * np.where(xx < EDGE, 0.25, 1.0))[..., None] * np.array([1.0, 0.75, 0.5, 0.0])
    irr = irr.astype(np.float16)
    for i, (x, y, value) in enumerate(NONFINITE_IRRADIANCE):
        irr[y, x, i % 3] = value
    return rays.view(np.uint16), irr.view(np.uint16), mv, previous_depth


def planted(frame, history, moments):
    """frame 1's history: the frame before's outputs with the planted texels"""
    if frame != 1:
        return history, moments
    history, moments = history.copy(), moments.copy()
    for x, y in NAN_HISTORY:
        history[y, x, 1] = np.nan
    for x, y in ZERO_COUNT:
        history[y, x, 3] = 0
    for x, y in INF_MOMENT:
        moments[y, x, 1] = np.inf
    return history, moments


def generate(seed):
    depth, normals, z = scene(seed)
    out = {"seed": np.int64(seed), "depth": depth, "normals": normals}
    history = moments = None
    for frame in range(FRAMES):
        rays, irr, mv, previous_depth = frame_inputs(frame, seed, depth, z)
        out[f"ray_buffer{frame}"], out[f"ray_irradiance{frame}"], out[f"motion_vectors{frame}"] = rays, irr, mv
        if frame:
            out[f"previous_depth{frame}"] = previous_depth
            history, moments = planted(frame, history, moments)
        for passes in range(4):
            accum, mom, drb, dirr = ref.denoise(rays, irr, depth, normals, mv, previous_depth if frame else None, history, moments, view(frame), params(frame, passes))
            out[f"denoised_irradiance{frame}_passes{passes}"] = dirr
        if frame == 0:
            out["denoised_ray_buffer0"] = drb  # (the unit normal and the input's distance: it does not depend on the frame's samples)
        out[f"accum{frame}"], out[f"moments{frame}"] = accum, mom
        history, moments = accum, mom
    return out


def frame_of(fx, frame):
    """the eight input planes of `frame` from a loaded (or generated) fixture; the previous-frame planes are None for frame 0"""
    history, moments = planted(frame, fx[f"accum{frame - 1}"], fx[f"moments{frame - 1}"]) if frame else (None, None)
    return dict(ray_buffer=fx[f"ray_buffer{frame}"], ray_irradiance=fx[f"ray_irradiance{frame}"], depth=fx["depth"], normals=fx["normals"],
                motion_vectors=fx[f"motion_vectors{frame}"], previous_depth=fx[f"previous_depth{frame}"] if frame else None, history=history,
                history_moments=moments)


if __name__ == "__main__":
    data = generate(69)
    np.savez_compressed(FIXTURE, **data)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; sample counts of frame 2: " + str(np.unique(data["accum2"][..., 3], return_counts=True)))
