"""Writes tests/golden/motion_blur_96x54.npz with the numpy restatement of sah_motion_blur (tests/motion_blur_ref.py): the input planes and
the output for each of CASES.

    python tools/gen_golden_motion_blur.py

The scene is analytic: a near box (z = 2) in front of a far wall (z = 10), textured so that any blur moves bits.  Two vector fields at the
render resolution 96 x 54 — six tiles by three and three eighths — formed analytically: a pan in which the box moves and the wall stands
(so the fixture holds a moving foreground over a static background and, with the roles swapped, the reverse), and a dolly towards the
scene, whose vectors grow from the centre and differ between box and wall.  The upscale case renders 64 x 36 and blurs at 96 x 54."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import motion_blur_ref as ref  # noqa: E402

WIDTH, HEIGHT = 96, 54
LOW = (64, 36)
FIXTURE = os.path.join(ROOT, "tests", "golden", f"motion_blur_{WIDTH}x{HEIGHT}.npz")
# (field, parameters): the fields are keys of inputs()
CASES = [("box_pan", dict()),
         ("wall_pan", dict()),
         ("dolly", dict()),
         ("box_pan", dict(sample_count=2)),
         ("dolly", dict(sample_count=32, max_blur_pixels=12.0)),
         ("box_pan", dict(flags=ref.DITHER)),
         ("dolly", dict(flags=ref.DITHER, shutter=1.0, depth_extent=0.25)),
         ("low", dict()),
         ("low", dict(flags=ref.DITHER, jitter=(0.25, -0.375), previous_jitter=(-0.125, 0.3125))),
         ("jittered_pan", dict(jitter=(0.25, -0.375), previous_jitter=(-0.125, 0.3125)))]


def _field(w, h, seed, kind):
    depth = ref.box_depth(w, h)
    box = ref.box_mask(w, h)
    if kind == "dolly":
        mv = ref.dolly_vectors(w, h, depth, 2.5)
    else:
        moving = box if kind == "box" else ~box
        g = np.random.default_rng(seed)
        vec = np.where(moving[..., None], np.array([22.0, -9.0]), 0.0) + g.normal(0.0, 0.02, (h, w, 2))  # (the noise: no two keys of a tile tie by accident)
        mv = ref.to_half_bits(vec)
    return depth, mv


def inputs(seed):
    out = {"scene": ref.textured_scene(WIDTH, HEIGHT, seed)}
    for name, (w, h, kind) in {"box_pan": (WIDTH, HEIGHT, "box"), "wall_pan": (WIDTH, HEIGHT, "wall"), "dolly": (WIDTH, HEIGHT, "dolly"),
                               "low": (LOW[0], LOW[1], "box")}.items():
        out[f"{name}_depth"], out[f"{name}_mv"] = _field(w, h, seed + len(name), kind)
    # the jittered pan: the box pan's vectors as a jittered frame carries them (jitter - previous_jitter added)
    shift = np.array([0.25, -0.375], ref.f32) - np.array([-0.125, 0.3125], ref.f32)
    out["jittered_pan_depth"] = out["box_pan_depth"]
    out["jittered_pan_mv"] = ref.to_half_bits(ref.h2f(out["box_pan_mv"]) + shift)
    return out


def generate(seed):
    data = inputs(seed)
    out = {"seed": np.int64(seed)}
    out.update(data)
    results, passed = [], []
    for field, params in CASES:
        o, info = ref.motion_blur_ex(data["scene"], data[f"{field}_depth"], data[f"{field}_mv"], **params)
        results.append(o)
        passed.append(info["passed"])
    out["out"] = np.stack(results)
    out["passed"] = np.packbits(np.stack(passed), axis=-1)
    return out


if __name__ == "__main__":
    data = generate(54)
    np.savez_compressed(FIXTURE, **data)
    changed = [(data["out"][i] != data["scene"]).any(-1).mean() for i in range(len(CASES))]
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; pixels that differ from scene, per case: " + ", ".join(f"{c:.3f}" for c in changed))
