"""Argument fuzz of the LPV geometry-volume entries (include/sah_lpv_gv.h) on a context without a device, in a child process (run by
tests/test_lpv_gv_cpu.py): the generators of tests/abi_fuzz_child.py, every call must come back with a sah_status code.

    python tests/gv_fuzz_child.py SEED ITERATIONS
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib  # noqa: E402
from tests.abi_fuzz_child import child_main  # noqa: E402


def make_calls(L, h, f):
    rgba16 = _abi.FORMAT_R16G16B16A16_SFLOAT

    def ctx():
        return None if f.g.random() < 0.03 else h

    def opt(obj, null_p=0.06):
        return f.ptr(obj, null_p)

    def ncasc():
        return int(f.pick([0, 1, 2, 3, 4, 4, 4, 5, 2 ** 31, 2 ** 32 - 1]))

    def cascades():
        a = (_abi.LpvCascadeMatrices * 4)()
        f.keep.append(a)
        return None if f.g.random() < 0.15 else a

    def vols3():
        a = (_abi.Volume * 3)(*[f.volume(rgba16, (128, 32, 32)) for _ in range(3)])
        f.keep.append(a)
        return None if f.g.random() < 0.1 else a

    def rsm():
        res = (int(f.pick([128, 128, 1, 7, 64])),) * 2
        return opt(_abi.RsmTargets(f.volume(43, res + (4,)), f.volume(_abi.FORMAT_R8G8B8A8_UNORM, res + (4,)), f.volume(_abi.FORMAT_D16_UNORM, res + (4,))))

    def scene_gv():
        s = f.extent(None)
        return L.sah_lpv_inject_scene_gv(ctx(), opt(f.plane(_abi.FORMAT_D32_SFLOAT, s)), opt(f.plane(rgba16, s)), opt(f.random_bits(_abi.ViewData)),
                                         cascades(), ncasc(), opt(f.volume(rgba16, (128, 32, 32))))

    return {
        "sah_lpv_inject_rsm_gv": lambda: L.sah_lpv_inject_rsm_gv(ctx(), rsm(), cascades(), f.u32((0, 0, 1, 3, 4)), f.u32((0, 1, 4, 4, 5)), ncasc(),
                                                                 opt(f.volume(rgba16, (128, 32, 32)))),
        "sah_lpv_inject_scene_gv": scene_gv,
        "sah_lpv_propagate_gv": lambda: L.sah_lpv_propagate_gv(ctx(), vols3(), vols3(), opt(f.volume(rgba16, (128, 32, 32)), 0.3), ncasc(),
                                                               int(f.pick([0, 1, 2, 3, 32]))),
    }


def main():
    return child_main(make_calls, lib.GV_EXPORTS, sys.argv)


if __name__ == "__main__":
    sys.exit(main())
