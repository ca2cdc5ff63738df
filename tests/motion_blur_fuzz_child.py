"""Argument fuzz of sah_motion_blur (include/sah_motion_blur.h) on a context without a device, in a child process (run by
tests/test_motion_blur_cpu.py): the generators of tests/abi_fuzz_child.py, NULLs and parameter blocks of random bits; every call must come
back with a sah_status code.

    python tests/motion_blur_fuzz_child.py SEED ITERATIONS
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib  # noqa: E402
from tests.abi_fuzz_child import child_main  # noqa: E402


def make_calls(L, h, f):
    nan, inf = float("nan"), float("inf")

    def params():
        r = f.g.random()
        if r < 0.05:
            return None
        if r < 0.35:
            return C.pointer(f.random_bits(_abi.MotionBlurParams))
        jit = lambda: (float(f.pick([0.0, 0.25, -0.5, inf, nan])), float(f.pick([0.0, 0.0, 0.375, -inf])))  # noqa: E731
        p = _abi.MotionBlurParams.default(shutter=float(f.pick([0.5, 0.5, 1.0, 0.0, 1.5, -1.0, inf, nan])), max_blur_pixels=float(f.pick([32.0, 32.0, 1.0, 0.0, 33.0, inf, nan])),
                                          min_velocity_pixels=float(f.pick([0.5, 0.0, -1.0, inf, nan])), sample_count=int(f.pick([12, 2, 32, 0, 1, 13, 34, 0xFFFFFFFF])),
                                          depth_extent=float(f.pick([1.0, 1e-6, 0.0, -1.0, inf, nan])), z_near=float(f.pick([0.1, 0.05, 0.0, -1.0, inf, nan])),
                                          jitter=jit(), previous_jitter=jit(), flags=int(f.pick([0, 1, 2, 3, 0x80000000])))
        f.keep.append(p)
        return C.pointer(p)

    def motion_blur():
        size = f.extent(None)
        low = f.pick([size, size, (max(1, size[0] * 2 // 3), max(1, size[1] * 2 // 3)), (size[0] + 1, size[1])])
        grid = ((low[0] + 15) // 16, (low[1] + 15) // 16)
        scene = f.plane(97, size)
        mv = f.plane(83, low)
        out = f.pick([f.plane(97, size), f.plane(97, size), f.plane(97, size), scene])
        tiles = f.pick([f.plane(83, grid), f.plane(83, grid), f.plane(83, grid), f.plane(83, low), mv])
        return L.sah_motion_blur(None if f.g.random() < 0.03 else h, f.ptr(scene), f.ptr(f.plane(126, low)), f.ptr(mv), f.ptr(tiles), f.ptr(out), params(),
                                 f.u32((0, 0, 1, 16)), f.u32((0, 0, 16, 64)))

    return {"sah_motion_blur": motion_blur}


def main():
    return child_main(make_calls, lib.MOTION_BLUR_EXPORTS, sys.argv)


if __name__ == "__main__":
    sys.exit(main())
