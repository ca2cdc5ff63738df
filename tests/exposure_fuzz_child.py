"""Argument fuzz of the auto-exposure entries (include/sah_exposure.h) on a context without a device, in a child process (run by
tests/test_exposure_cpu.py): the generators of tests/abi_fuzz_child.py, NULLs and parameter blocks of random bits; every call must come
back with a sah_status code.

    python tests/exposure_fuzz_child.py SEED ITERATIONS
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib  # noqa: E402
from tests.abi_fuzz_child import child_main  # noqa: E402


def make_calls(L, h, f):
    rgba16 = _abi.FORMAT_R16G16B16A16_SFLOAT

    def ctx():
        return None if f.g.random() < 0.03 else h

    def device_address(null_p=0.06):
        return None if f.g.random() < null_p else C.c_void_p(f.addr())

    def params():
        r = f.g.random()
        if r < 0.06:
            return None
        if r < 0.4:
            return C.pointer(f.random_bits(_abi.ExposureParams))
        p = _abi.ExposureParams.default(flags=int(f.pick([0, 0, 1, 1, 2, 3, 0x80000000])), max_workgroups=f.u32((0, 0, 1, 7)),
                                        adaptation=float(f.pick([1.0, 0.25, 0.0, -1.0, 2.0, float("nan")])))
        f.keep.append(p)
        return C.pointer(p)

    def meter():
        size = f.extent(None)
        scene = f.plane(rgba16, size)
        out = f.pick([None, None, f.plane(rgba16, size), scene])
        state = device_address()
        return L.sah_exposure_meter(ctx(), f.ptr(scene), f.pick([state, device_address(0.3)]), state, device_address(),
                                    None if out is None else f.ptr(out), params())

    def apply():
        size = f.extent(None)
        scene = f.plane(rgba16, size)
        out = f.pick([f.plane(rgba16, size), scene])
        return L.sah_exposure_apply(ctx(), f.ptr(scene), device_address(), f.ptr(out), f.u32((0, 0, 1, 16)), f.u32((0, 0, 16, 64)))

    return {"sah_exposure_meter": meter, "sah_exposure_apply": apply}


def main():
    return child_main(make_calls, lib.EXPOSURE_EXPORTS, sys.argv)


if __name__ == "__main__":
    sys.exit(main())
