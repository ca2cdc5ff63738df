"""Argument fuzz of the LPV geometry-volume entries (include/sah_lpv_gv.h) on a context without a device, in a child process (run by
tests/test_lpv_gv_cpu.py): the generators of tests/abi_fuzz_child.py, every call must come back with a sah_status code.

    python tests/gv_fuzz_child.py SEED ITERATIONS
"""
import collections
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib  # noqa: E402
from tests.abi_fuzz_child import STATUS, Fuzz, _abi_name  # noqa: E402


def main():
    seed, iterations = int(sys.argv[1]), int(sys.argv[2])
    L = lib.load()
    L.sah_debug_create_detached.argtypes = [C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    rc = L.sah_debug_create_detached(C.byref(h))
    if rc == _abi.SAH_ERR_UNSUPPORTED:
        print("SKIP: a HIP device is present (the fuzz's made-up addresses must not reach a GPU)")
        return 0
    assert rc == 0 and h.value, rc
    f = Fuzz(seed)
    seen = collections.defaultdict(collections.Counter)
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

    calls = {
        "sah_lpv_inject_rsm_gv": lambda: L.sah_lpv_inject_rsm_gv(ctx(), rsm(), cascades(), f.u32((0, 0, 1, 3, 4)), f.u32((0, 1, 4, 4, 5)), ncasc(),
                                                                 opt(f.volume(rgba16, (128, 32, 32)))),
        "sah_lpv_inject_scene_gv": scene_gv,
        "sah_lpv_propagate_gv": lambda: L.sah_lpv_propagate_gv(ctx(), vols3(), vols3(), opt(f.volume(rgba16, (128, 32, 32)), 0.3), ncasc(),
                                                               int(f.pick([0, 1, 2, 3, 32]))),
    }
    uncovered = sorted(set(lib.GV_EXPORTS) - set(calls))
    assert not uncovered, f"entry points without a fuzz case: {uncovered}"
    for i in range(iterations):
        for name in sorted(calls):
            rc = calls[name]()
            if rc not in STATUS:
                print(f"FAIL: {name} returned {rc}, not a sah_status (iteration {i}, seed {seed})")
                return 1
            seen[name][rc] += 1
        f.keep.clear()
    L.sah_destroy(h)
    for name in sorted(calls):
        print(f"{name:26s} " + "  ".join(f"{_abi_name(rc)}: {n}" for rc, n in sorted(seen[name].items(), reverse=True)))
    print(f"OK: {iterations} iterations x {len(calls)} entry points, seed {seed}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
