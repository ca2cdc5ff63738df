"""Argument fuzz of sah_motion_vectors_render (include/sah_motion_vectors.h) on a context without a device, in a child process (run by
tests/test_motion_vectors_cpu.py): the generators of tests/abi_fuzz_child.py.  The child restates the header's argument contract: a
malformed call must answer SAH_ERR_INVALID_ARGUMENT, a well-formed one gets as far as selecting the device, which a detached context
does not have (SAH_ERR_HIP) — so nothing is ever launched.

    python tests/mv_fuzz_child.py SEED ITERATIONS
"""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib  # noqa: E402
from tests.abi_fuzz_child import Fuzz, _abi_name  # noqa: E402

MAX_EXTENT = 8192


def scene_ok(s):
    if s.num_primitives == 0:
        return True
    return bool(s.primitives and s.indices and s.vertex_positions) and s.num_primitives < (1 << 24)


def plane_ok(p, fmt, w, h):
    return bool(p.ptr) and p.format == fmt and (p.width, p.height) == (w, h) and p.row_pitch_bytes >= w * 4 and p.ptr % 4 == 0 and p.row_pitch_bytes % 4 == 0


def main():
    seed, iterations = int(sys.argv[1]), int(sys.argv[2])
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        print("SKIP: a HIP device is present (the fuzz's made-up addresses must not reach a GPU)")
        return 0
    f = Fuzz(seed)
    seen = collections.Counter()
    for i in range(iterations):
        ctx = None if f.g.random() < 0.03 else h
        size = f.extent(None)
        scene, view = f.scene(), f.random_bits(_abi.ViewData)
        depth, mv = f.plane(_abi.FORMAT_D32_SFLOAT, size), f.plane(_abi.FORMAT_R16G16_SFLOAT, size)
        args = [f.ptr(scene), f.ptr(view), f.ptr(depth), f.ptr(mv)]
        well_formed = (ctx is not None and all(a is not None for a in args) and scene_ok(scene) and 0 < depth.width <= MAX_EXTENT and
                       0 < depth.height <= MAX_EXTENT and plane_ok(depth, _abi.FORMAT_D32_SFLOAT, depth.width, depth.height) and
                       plane_ok(mv, _abi.FORMAT_R16G16_SFLOAT, depth.width, depth.height))
        want = _abi.SAH_ERR_HIP if well_formed else _abi.SAH_ERR_INVALID_ARGUMENT
        rc = L.sah_motion_vectors_render(ctx, *args, f.addr())
        if rc != want:
            print(f"FAIL: sah_motion_vectors_render returned {rc}, expected {want} (iteration {i}, seed {seed}): depth {depth.width}x{depth.height} "
                  f"fmt {depth.format} pitch {depth.row_pitch_bytes} ptr {depth.ptr}, target {mv.width}x{mv.height} fmt {mv.format} pitch {mv.row_pitch_bytes} ptr {mv.ptr}")
            return 1
        seen[rc] += 1
        f.keep.clear()
    L.sah_destroy(h)
    print("sah_motion_vectors_render  " + "  ".join(f"{_abi_name(rc)}: {n}" for rc, n in sorted(seen.items(), reverse=True)))
    if seen[_abi.SAH_ERR_HIP] == 0 or seen[_abi.SAH_ERR_INVALID_ARGUMENT] == 0:
        print("FAIL: the fuzz produced only one kind of call")
        return 1
    print(f"OK: {iterations} iterations, seed {seed}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
