"""Argument fuzz of sah_sharpen (include/sah_sharpen.h) on a context without a device, in a child process (run by
tests/test_sharpen_cpu.py): the generators of tests/abi_fuzz_child.py, NULLs and parameter blocks of random bits; every call must come back
with a sah_status code.

    python tests/sharpen_fuzz_child.py SEED ITERATIONS
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

    def params():
        r = f.g.random()
        if r < 0.06:
            return None
        if r < 0.4:
            return C.pointer(f.random_bits(_abi.SharpenParams))
        p = _abi.SharpenParams.default(flags=int(f.pick([0, 0, 1, 1, 2, 3, 0x80000000])), sharpness=float(f.pick([1.0, 0.5, 0.0, -1.0, 2.0, float("nan")])),
                                       pre_scale=float(f.pick([1.0, 0.25, 0.0, -1.0, float("inf"), float("nan")])))
        f.keep.append(p)
        return C.pointer(p)

    def sharpen():
        size = f.extent(None)
        scene = f.plane(rgba16, size)
        out = f.pick([f.plane(rgba16, size), f.plane(rgba16, size), scene])
        exposure = None if f.g.random() < 0.4 else C.c_void_p(f.addr())
        return L.sah_sharpen(None if f.g.random() < 0.03 else h, f.ptr(scene), exposure, f.ptr(out), params(), f.u32((0, 0, 1, 16)), f.u32((0, 0, 16, 64)))

    calls = {"sah_sharpen": sharpen}
    uncovered = sorted(set(lib.SHARPEN_EXPORTS) - set(calls))
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
