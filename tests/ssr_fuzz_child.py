"""Argument fuzz of sah_ssr (include/sah_ssr.h) on a context without a device, in a child process (run by tests/test_ssr_cpu.py): the
generators of tests/abi_fuzz_child.py, NULLs, view and parameter blocks of random bits; every call must come back with a sah_status code.

    python tests/ssr_fuzz_child.py SEED ITERATIONS
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib  # noqa: E402
from tests.abi_fuzz_child import child_main  # noqa: E402


def make_calls(L, h, f):
    nan, inf = float("nan"), float("inf")

    def view():
        r = f.g.random()
        if r < 0.05:
            return None
        if r < 0.35:
            return C.pointer(f.random_bits(_abi.ViewData))
        v = _abi.ViewData()
        for i in (0, 5, 10, 15):
            v.view[i] = 1.0
        v.projection[0], v.projection[5], v.z_near = 1.0, 1.7, float(f.pick([0.05, 0.05, 0.05, 0.0, -1.0, inf, nan]))
        f.keep.append(v)
        return C.pointer(v)

    def params():
        r = f.g.random()
        if r < 0.05:
            return None
        if r < 0.35:
            return C.pointer(f.random_bits(_abi.SsrParams))
        p = _abi.SsrParams.default(max_distance=float(f.pick([50.0, 50.0, 1e-3, 0.0, -1.0, inf, nan])), thickness=float(f.pick([0.5, 0.0, inf, -1.0, nan])),
                                   stride_pixels=float(f.pick([4.0, 1.0, 2.5, 0.5, inf, nan])), max_steps=int(f.pick([64, 1, 256, 0, 257, 0xFFFFFFFF])),
                                   refine_steps=int(f.pick([4, 0, 8, 9, 0xFFFFFFFF])), max_roughness=float(f.pick([0.6, 1.0, 0.0, 1.5, nan])),
                                   edge_fade=float(f.pick([0.1, 0.5, 0.0, 0.6, nan])), intensity=float(f.pick([1.0, 0.0, -1.0, inf, nan])),
                                   flags=int(f.pick([0, 1, 2, 3, 4, 0x80000000])))
        f.keep.append(p)
        return C.pointer(p)

    def ssr():
        size = f.extent(None)
        blocks = ((size[0] + 7) // 8, (size[1] + 7) // 8)
        source = f.plane(97, size)
        lit = f.pick([f.plane(97, size), source])
        out = f.pick([f.plane(97, size), f.plane(97, size), f.plane(97, size), lit])
        scratch = f.plane(100, f.pick([blocks, blocks, blocks, size]))
        return L.sah_ssr(None if f.g.random() < 0.03 else h, view(), f.ptr(f.plane(43, size)), f.ptr(f.plane(97, size)), f.ptr(f.plane(37, size)),
                         f.ptr(f.plane(126, size)), f.ptr(source), f.ptr(lit), f.ptr(scratch), f.ptr(out), params(), f.u32((0, 0, 1, 16)), f.u32((0, 0, 16, 64)))

    return {"sah_ssr": ssr}


def main():
    return child_main(make_calls, lib.SSR_EXPORTS, sys.argv)


if __name__ == "__main__":
    sys.exit(main())
