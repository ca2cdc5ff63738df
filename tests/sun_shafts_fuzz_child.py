"""Argument fuzz of sah_sun_shafts (include/sah_sun_shafts.h) on a context without a device, in a child process (run by
tests/test_sun_shafts_cpu.py): the generators of tests/abi_fuzz_child.py, NULLs, views and suns and parameter blocks of random bits; every
call must come back with a sah_status code.

    python tests/sun_shafts_fuzz_child.py SEED ITERATIONS
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
            return C.pointer(f.random_bits(_abi.SunShaftsParams))
        rgb = lambda: tuple(float(f.pick([1.0, 0.0, 3e-4, -1.0, inf, nan])) for _ in range(3))  # noqa: E731
        p = _abi.SunShaftsParams.default(step_length=float(f.pick([0.5, 0.5, 1e-3, 0.0, -1.0, inf, nan])), num_steps=int(f.pick([32, 1, 64, 0, 65, 0xFFFFFFFF])),
                                         step_transmittance=float(f.pick([0.98, 1.0, 1e-6, 0.0, 1.5, -1.0, inf, nan])), albedo=rgb(), ambient=rgb(),
                                         anisotropy=float(f.pick([0.6, 0.0, -0.9, 1.0, -1.0, inf, nan])), depth_bias=float(f.pick([0.0005, 0.0, -1.0, inf, nan])),
                                         depth_sharpness=float(f.pick([50.0, 0.0, -1.0, inf, nan])), downscale=int(f.pick([1, 2, 1, 2, 0, 3, 0xFFFFFFFF])),
                                         dither_offset=int(f.pick([0, 5, 15, 16, 0xFFFFFFFF])), flags=int(f.pick([0, 1, 2, 3, 4, 0x80000000])))
        f.keep.append(p)
        return C.pointer(p)

    def sun_shafts():
        size = f.extent(None)
        grid = f.pick([((size[0] + 1) // 2, (size[1] + 1) // 2), size, size])
        lit = f.plane(97, size)
        out = f.pick([f.plane(97, size), f.plane(97, size), f.plane(97, size), lit])
        march = f.pick([f.plane(97, grid), f.plane(97, grid), lit])
        view, sun = f.random_bits(_abi.ViewData), f.random_bits(_abi.SunLightConstants)
        if f.g.random() < 0.8:
            view.z_near = float(f.pick([0.05, 0.1, 0.0, -1.0, inf, nan]))
        shadowmap = f.volume(int(f.pick([124, 126, 124, 126, 97])), like=(int(f.pick([64, 8, 4096])), 64, int(f.pick([4, 1, 3, 0, 9]))))
        return L.sah_sun_shafts(None if f.g.random() < 0.03 else h, f.ptr(view), f.ptr(sun), f.ptr(shadowmap, 0.2), f.ptr(f.plane(126, size)), f.ptr(lit),
                                f.ptr(march), f.ptr(out), params(), f.u32((0, 0, 1, 16)), f.u32((0, 0, 16, 64)))

    return {"sah_sun_shafts": sun_shafts}


def main():
    return child_main(make_calls, lib.SUN_SHAFTS_EXPORTS, sys.argv)


if __name__ == "__main__":
    sys.exit(main())
