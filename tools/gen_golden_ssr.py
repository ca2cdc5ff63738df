"""Writes tests/golden/ssr_96x54.npz with the numpy restatement of sah_ssr (tests/ssr_ref.py): the input planes of one frame and the output
for each of CASES.

    python tools/gen_golden_ssr.py

96 x 54 is three workgroup tiles of the trace kernel (32 x 8) across and six and three quarters down, twelve 8 x 8 blocks by six and three
quarters.  Columns 0 .. 71 are the analytic mirror room of tests/ssr_ref.py (a metal floor, a striped back wall, sky above it) with unclean
source texels planted on the wall where floor pixels reflect them; columns 72 .. 95 are a random G-buffer with sky, NaN, negative and infinite
depths and zero / NaN normals.  tests/test_ssr_cpu.py asserts that the frame takes every branch it is there for."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ssr_ref  # noqa: E402

WIDTH, HEIGHT, SPLIT = 96, 54, 72
FIXTURE = os.path.join(ROOT, "tests", "golden", f"ssr_{WIDTH}x{HEIGHT}.npz")
PLANES = ("color", "normals", "data", "depth", "source", "lit")
CASES = [dict(thickness=2.0, stride_pixels=2.0, max_steps=128),
         dict(thickness=2.0, stride_pixels=4.0, max_steps=64, flags=ssr_ref.JITTER),
         dict(thickness=0.5, stride_pixels=1.0, max_steps=256, refine_steps=8, flags=ssr_ref.REFLECTION_ONLY, intensity=0.5, edge_fade=0.25),
         dict(thickness=3e38, stride_pixels=2.5, max_steps=7, refine_steps=0, max_roughness=1.0, max_distance=3.0)]
UNCLEAN = [(20, 22, 0, 0x7e00), (21, 23, 1, 0x7c00), (40, 24, 2, 0xbc00), (41, 25, 0, 0xfc00)]  # (x, y, channel, bits) on the wall: NaN, +inf, -1, -inf


def view():
    return ssr_ref.room_view()


def inputs(seed):
    frame, _ = ssr_ref.mirror_room(WIDTH, HEIGHT, seed)
    noise = ssr_ref.random_frame(WIDTH, HEIGHT, seed)
    for k in PLANES:
        frame[k] = np.array(frame[k])
        frame[k][:, SPLIT:] = noise[k][:, SPLIT:]
    for x, y, c, bits in UNCLEAN:
        frame["source"][y, x, c] = bits
    return frame


def generate(seed):
    frame = inputs(seed)
    out = {"seed": np.int64(seed)}
    out.update(frame)
    out["out"] = np.stack([ssr_ref.ssr(view=view(), params=p, **frame) for p in CASES])
    return out


if __name__ == "__main__":
    data = generate(96)
    np.savez_compressed(FIXTURE, **data)
    changed = [(data["out"][i][..., :3] != data["lit"][..., :3]).any(-1).mean() for i in range(len(CASES))]
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; pixels whose rgb differs from lit, per case: " + ", ".join(f"{c:.3f}" for c in changed))
