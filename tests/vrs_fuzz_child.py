"""Argument fuzz of sah_lighting_vrs and sah_vrsaa_resolve (include/sah_vrs.h) on a context without a device, in a child process (run by
tests/test_lighting_vrs_cpu.py): the generators of tests/abi_fuzz_child.py — its lighting descriptors among them —, NULLs, texel sizes and
tolerances of every kind; every call must come back with a sah_status code.

    python tests/vrs_fuzz_child.py SEED ITERATIONS
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib  # noqa: E402
from tests.abi_fuzz_child import child_main  # noqa: E402


def make_calls(L, h, f):
    rgba16 = _abi.FORMAT_R16G16B16A16_SFLOAT

    def lighting_vrs():
        if f.g.random() < 0.03:
            return L.sah_lighting_vrs(h, None)
        d = f.lighting_desc()
        if f.g.random() < 0.6:  # what the entry supports, so that its own checks are reached
            d.lights, d.row_begin, d.row_end = None, int(f.pick([0, 0, 4, 6])), int(f.pick([0, 0, 8, 9]))
            if d.gi and f.g.random() < 0.8:
                d.gi.contents.kind = int(f.pick([_abi.GI_NONE, _abi.GI_LPV]))
        size = (d.lit.contents.width, d.lit.contents.height) if d.lit else (64, 64)
        texel = (f.u32((4, 8, 16, 32, 64, 64, 0, 2, 12, 128)), f.u32((4, 8, 16, 32, 64, 64, 0, 3, 24, 128)))
        like = tuple(-(-s // max(1, t)) + int(f.pick([0, 0, 0, 1, -1])) for s, t in zip(size, texel))
        sri = f.plane(_abi.FORMAT_R8_UINT, tuple(max(0, v) & 0xFFFFFFFF for v in like))
        v = _abi.LightingVrsDesc(f.ptr(d), f.ptr(sri), (C.c_uint32 * 2)(*texel), float(f.pick([0.0, 0.01, 1.0, float("inf"), -0.5, float("nan"), -0.0])))
        f.keep.append(v)
        return L.sah_lighting_vrs(None if f.g.random() < 0.03 else h, C.byref(v))

    def resolve():
        w, hh = f.extent(None)
        lit = f.plane(rgba16, f.pick([(2 * w, 2 * hh), (2 * w, 2 * hh), (2 * w + 1, 2 * hh), (w, hh), (2 * w, 4 * hh)]))
        out = f.pick([f.plane(rgba16, (w, hh)), f.plane(rgba16, (w, hh)), lit])
        return L.sah_vrsaa_resolve(None if f.g.random() < 0.03 else h, f.ptr(lit), f.ptr(out), f.u32((0, 0, 1, 16)), f.u32((0, 0, 16, 64)))

    return {"sah_lighting_vrs": lighting_vrs, "sah_vrsaa_resolve": resolve}


def main():
    return child_main(make_calls, lib.VRS_EXPORTS, sys.argv)


if __name__ == "__main__":
    sys.exit(main())
