"""Writes tests/golden/sun_shafts_96x54.npz: the inputs of a small frame in the atrium's camera — the view and the sun as the bytes of their
structures, a box-and-wall depth with sky texels, a lit plane, a D16 and a D32 shadow map of blocky noise — and, for each of CASES, the
`out` and `march` planes the numpy restatement (tests/sun_shafts_ref.py) gives.  The fixture pins include/sah_sun_shafts.h bit for bit:
tests/test_sun_shafts_cpu.py holds the restatement to it, tests/test_sun_shafts_gpu.py the device.

    python tools/gen_golden_sun_shafts.py          # rewrites the fixture (only when the header's arithmetic changes)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import sun_shafts_ref as ref  # noqa: E402

WIDTH, HEIGHT = 96, 54
FIXTURE = os.path.join(ROOT, "tests", "golden", f"sun_shafts_{WIDTH}x{HEIGHT}.npz")
MEDIUM = dict(albedo=(3e-4, 2.5e-4, 2e-4), ambient=(0.02, 0.03, 0.05))
# (shadow map, settings)
CASES = [("d16", dict(MEDIUM)),
         ("d16", dict(MEDIUM, downscale=2, flags=ref.DITHER, dither_offset=5)),
         ("d32", dict(MEDIUM, num_steps=64, step_length=0.25, step_transmittance=0.97, anisotropy=-0.3, flags=ref.DITHER)),
         ("d32", dict(MEDIUM, downscale=2, num_steps=17, step_length=1.5, depth_sharpness=4.0, flags=ref.TERM_ONLY)),
         ("none", dict(MEDIUM, num_steps=8, step_transmittance=0.9, anisotropy=0.0))]


def inputs():
    view = ref.scene_view(WIDTH, HEIGHT)
    sun = ref.scene_sun(view)
    return dict(view=np.frombuffer(bytes(view.gpu_data), np.uint8).copy(), sun=np.frombuffer(bytes(sun), np.uint8).copy(),
                depth=ref.box_depth(WIDTH, HEIGHT), lit=ref.textured_lit(WIDTH, HEIGHT, 1), map_d16=ref.noise_map(4, 64, 3, block=4),
                map_d32=ref.noise_map(3, 32, 4, np.float32, block=2))


def structures(fx):
    """the view and the sun of a loaded fixture as their ctypes structures"""
    from androidrenderer_amd import _abi
    return _abi.ViewData.from_buffer_copy(fx["view"].tobytes()), _abi.SunLightConstants.from_buffer_copy(fx["sun"].tobytes())


def shadow_map(fx, name):
    return None if name == "none" else fx[f"map_{name}"]


def outputs(fx):
    view, sun = structures(fx)
    out, march = [], []
    for name, settings in CASES:
        o, info = ref.sun_shafts_ex(view, sun, shadow_map(fx, name), fx["depth"], fx["lit"], **settings)
        out.append(o)
        march.append(info["bits"])
    return out, march


def main():
    fx = inputs()
    out, march = outputs(fx)
    fx["out"] = np.stack(out)
    for i, m in enumerate(march):  # (two extents: not one array)
        fx[f"march{i}"] = m
    np.savez_compressed(FIXTURE, **fx)
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    assert C.sizeof(C.c_float) == 4
    main()
