"""Writes tests/golden/ssao_69x21.npz with the numpy restatement of sah_ssao (tests/ssao_ref.py): the inputs, and the output for blur_passes
0, 1 and 2 from the same inputs.

    python tools/gen_golden_ssao.py

69 x 21 is one tile of the raw kernel (64 x 16) plus five pixels in each axis, and two tiles of the blur kernel (32 x 16) plus five and one
plus five.  The planes are stored with the padded pitch they were generated with (depth: 72 texels, normals: 70), the padding holding a
pattern no texel has.  Three bands of columns: a near one (z about 1: the sampling radius capped at max_radius_pixels = 12), a middle one
(z 2 .. 6: uncapped, no fade) and a far one (z 18 .. 45: one pixel of radius, the fade strictly between 0 and 1 and at 0).  In the middle
band lies a block of sky with six lone far surface texels inside it (every tap of theirs is skipped: n == 0); in the near band a patch of
constant depth (blur weights of exactly 1).  NaN, negative and infinite depths and zero and NaN normals are planted at fixed places.
shadow_multiplier = 8 against shadow_clamp = 0.5 makes the clamp bite.  tests/test_ssao_cpu.py asserts that each planted case takes its
branch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ssao_ref  # noqa: E402

WIDTH, HEIGHT = ssao_ref.RAW_TILE[0] + 5, ssao_ref.RAW_TILE[1] + 5
DEPTH_PITCH, NORMALS_PITCH = 72, 70  # in texels
FIXTURE = os.path.join(ROOT, "tests", "golden", f"ssao_{WIDTH}x{HEIGHT}.npz")
f32 = np.float32
PARAMS = dict(radius=0.5, max_radius_pixels=12.0, shadow_multiplier=8.0, shadow_clamp=0.5, horizon_angle_threshold=0.06, fade_out_from=5.0,
              fade_out_to=30.0, edge_sharpness=50.0, flags=0)
PROJECTION = dict(p00=1.0, p11=2.0, p20=0.01, p21=-0.02, z_near=0.05)
_c, _s = np.cos(0.3), np.sin(0.3)
VIEW3 = np.array([[_c, 0.0, _s], [0.0, 1.0, 0.0], [-_s, 0.0, _c]], f32)  # view3[row][column]: a turn about y
SKY = (slice(6, 15), slice(30, 40))
LONE = [(32, 8), (35, 8), (38, 8), (32, 11), (35, 11), (38, 11)]  # (x, y) inside SKY, all eight neighbours sky
FLAT = (slice(15, 20), slice(5, 12))
NAN_DEPTH = [(3, 3), (20, 10), (27, 17), (44, 3), (50, 9), (60, 15)]
NEGATIVE_DEPTH = [(8, 7), (15, 2), (26, 5), (43, 18), (55, 4), (64, 12)]
INF_DEPTH = [(12, 12), (48, 16)]
ZERO_NORMAL = [(2, 9), (18, 5), (25, 12), (42, 8), (52, 14), (66, 6)]
NAN_NORMAL = [(6, 2), (21, 16), (28, 3), (45, 13), (57, 10), (62, 18)]


def view():
    return ssao_ref.View.of(view3=VIEW3, **PROJECTION)


def inputs(seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH]
    bumps = np.sin(xx * 0.9) * np.cos(yy * 0.7)
    near = 1.0 + 0.06 * bumps + g.uniform(0, 0.01, (HEIGHT, WIDTH))
    middle = 4.0 + 1.5 * bumps + g.uniform(0, 0.4, (HEIGHT, WIDTH))
    far = 31.0 + 13.0 * np.sin(xx * 0.45 + yy * 0.3) + g.uniform(0, 0.5, (HEIGHT, WIDTH))
    z = np.where(xx < 24, near, np.where(xx < 46, middle, far))
    depth = (PROJECTION["z_near"] / z).astype(f32)
    depth[SKY] = 0.0
    for x, y in LONE:
        depth[y, x] = f32(PROJECTION["z_near"] / 40.0)
    depth[FLAT] = f32(0.05)
    for x, y in NAN_DEPTH:
        depth[y, x] = np.nan
    for x, y in NEGATIVE_DEPTH:
        depth[y, x] = -0.25
    for x, y in INF_DEPTH:
        depth[y, x] = np.inf
    n_view = np.concatenate([g.normal(0, 0.4, (HEIGHT, WIDTH, 2)), np.ones((HEIGHT, WIDTH, 1))], -1) * g.uniform(0.5, 2.0, (HEIGHT, WIDTH, 1))
    n_world = n_view @ VIEW3.astype(np.float64)  # the transpose of the turn applied to a column vector
    normals = np.concatenate([n_world, g.uniform(0, 1, (HEIGHT, WIDTH, 1))], -1).astype(np.float16)
    for x, y in ZERO_NORMAL:
        normals[y, x, :3] = 0.0
    for i, (x, y) in enumerate(NAN_NORMAL):
        normals[y, x, i % 3] = np.nan
    depth_plane = np.full((HEIGHT, DEPTH_PITCH), np.uint32(0xA5A5A5A5)).view(f32)
    depth_plane[:, :WIDTH] = depth
    normals_plane = np.full((HEIGHT, NORMALS_PITCH, 4), np.uint16(0xA5A5))
    normals_plane[:, :WIDTH] = normals.view(np.uint16)
    return depth_plane, normals_plane


def generate(seed):
    depth_plane, normals_plane = inputs(seed)
    depth, normals = depth_plane[:, :WIDTH], normals_plane[:, :WIDTH]
    out = {"seed": np.int64(seed), "width": np.int64(WIDTH), "depth_plane": depth_plane, "normals_plane": normals_plane,
           "params": np.array([PARAMS[k] for k in sorted(PARAMS)], f32), "projection": np.array([PROJECTION[k] for k in sorted(PROJECTION)], f32),
           "view3": VIEW3}
    for passes in (0, 1, 2):
        out[f"ao_blur{passes}"] = ssao_ref.ssao(depth, normals, view(), dict(PARAMS, blur_passes=passes))
    return out


if __name__ == "__main__":
    data = generate(69)
    np.savez_compressed(FIXTURE, **data)
    ao = data["ao_blur0"]
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; raw AO min {float(ao.min()):.4f}, below 1 at {int((ao < 1).sum())} of {ao.size}; "
          f"blurred twice: min {float(data['ao_blur2'].min()):.4f}")
