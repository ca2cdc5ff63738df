"""Argument fuzz of sah_translucent_render (include/sah_translucent.h) on a context without a device, in a child process (run by
tests/test_translucent_cpu.py): the generators of tests/abi_fuzz_child.py — its lighting descriptors and scenes among them — and NULLs;
every call must come back with a sah_status code.

    python tests/translucent_fuzz_child.py SEED ITERATIONS
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib  # noqa: E402
from tests.abi_fuzz_child import child_main  # noqa: E402


def make_calls(L, h, f):

    def translucent_render():
        if f.g.random() < 0.03:
            return L.sah_translucent_render(h, None)
        d = f.lighting_desc()
        if f.g.random() < 0.6:  # what the entry supports, so that its own checks are reached
            d.lights, d.row_begin, d.row_end = None, int(f.pick([0, 0, 4, 6])), int(f.pick([0, 0, 8, 9]))
            if d.gi and f.g.random() < 0.8:
                d.gi.contents.kind = int(f.pick([_abi.GI_NONE, _abi.GI_LPV]))
            if d.sun and f.g.random() < 0.8:
                d.sun.contents.shadow_mode = int(f.pick([_abi.SHADOW_MODE_OFF, _abi.SHADOW_MODE_CSM]))
        if d.gbuffer and d.lit and f.g.random() < 0.1:  # lit on top of the depth plane
            d.lit.contents.ptr = d.gbuffer.contents.depth.ptr
        scene = f.scene()
        t = _abi.TranslucentDesc(f.ptr(d), f.ptr(scene), C.c_void_p(f.addr() if f.g.random() < 0.5 else None))
        f.keep.append(t)
        return L.sah_translucent_render(None if f.g.random() < 0.03 else h, C.byref(t))

    return {"sah_translucent_render": translucent_render}


def main():
    return child_main(make_calls, lib.TRANSLUCENT_EXPORTS, sys.argv)


if __name__ == "__main__":
    sys.exit(main())
