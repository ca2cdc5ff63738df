"""Argument fuzz of sah_rtgi_denoise (include/sah_rtgi_denoise.h) on a context without a device, in a child process (run by
tests/test_rtgi_denoise_cpu.py): the generators of tests/abi_fuzz_child.py, NULLs, view and parameter blocks of random bits; every call
must come back with a sah_status code.

    python tests/rtgi_denoise_fuzz_child.py SEED ITERATIONS
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib  # noqa: E402
from tests.abi_fuzz_child import child_main  # noqa: E402

FORMATS = dict(ray_buffer=97, ray_irradiance=97, depth=126, normals=97, motion_vectors=83, previous_depth=126, history=109, history_moments=103,
               accum_out=109, moments_out=103, denoised_ray_buffer=97, denoised_irradiance=97)


def make_calls(L, h, f):
    assert list(FORMATS) == list(_abi.RtgiDenoiseDesc.PLANES)
    f.wild = 0.03  # twelve planes a call: with the generators' usual 0.1 no call would get past the plane checks

    def view():
        r = f.g.random()
        if r < 0.04:
            return None
        if r < 0.3:
            return C.pointer(f.random_bits(_abi.ViewData))
        v = _abi.ViewData()
        for i in (0, 5, 10, 15):
            v.view[i] = v.inverse_view[i] = v.last_frame_view[i] = 1.0
        v.projection[0], v.projection[5], v.z_near = 1.2, -2.0, float(f.pick([0.05] * 12 + [0.0, -1.0, float("nan"), float("inf")]))
        f.keep.append(v)
        return C.pointer(v)

    def params():
        r = f.g.random()
        if r < 0.04:
            return None
        if r < 0.35:
            return C.pointer(f.random_bits(_abi.RtgiDenoiseParams))
        if r < 0.65:
            p = _abi.RtgiDenoiseParams.default(flags=int(f.pick([0, 1])), passes=int(f.pick([0, 1, 2, 3])))
            f.keep.append(p)
            return C.pointer(p)
        p = _abi.RtgiDenoiseParams.default(flags=int(f.pick([0, 0, 1, 1, 2, 3, 0x80000000])), passes=f.u32((0, 1, 2, 3, 3, 4)),
                                           normal_squarings=f.u32((0, 5, 7, 8)), max_history=float(f.pick([32.0, 1.0, 0.0, 300.0, float("nan")])),
                                           min_history=float(f.pick([4.0, 1.0, 0.5, float("inf")])),
                                           luminance_sigma=float(f.pick([4.0, 0.0, -1.0, float("nan")])),
                                           luminance_floor=float(f.pick([1e-6, 0.0, float("inf")])))
        f.keep.append(p)
        return C.pointer(p)

    def desc():
        r = f.g.random()
        if r < 0.04:
            return None
        size = f.extent(None)  # (the descriptor's twelve pointers are host pointers the entry follows: random planes behind them, not random bits in them)
        planes = {}
        for name, fmt in FORMATS.items():
            if f.g.random() < 0.01:
                planes[name] = None
            elif f.g.random() < 0.01 and planes:
                planes[name] = f.pick([p for p in planes.values() if p is not None] or [f.plane(fmt, size)])  # another plane's memory
            else:
                planes[name] = f.plane(fmt, size)
        d = _abi.RtgiDenoiseDesc.of(**planes)
        f.keep.append(d)
        return C.pointer(d)

    def denoise():
        return L.sah_rtgi_denoise(None if f.g.random() < 0.03 else h, view(), desc(), params(), f.u32((0, 0, 0, 3, 16)), f.u32((0, 0, 9, 16, 64)))

    return {"sah_rtgi_denoise": denoise}


def main():
    return child_main(make_calls, lib.RTGI_DENOISE_EXPORTS, sys.argv)


if __name__ == "__main__":
    sys.exit(main())
