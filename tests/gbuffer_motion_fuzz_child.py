"""Argument fuzz of sah_gbuffer_motion_render (include/sah_gbuffer_motion.h) on a context without a device, in a child process (run by
tests/test_gbuffer_motion_cpu.py): the generators of tests/abi_fuzz_child.py, in the pattern of tests/mv_fuzz_child.py.  The child restates
the header's argument contract — the union of sah_gbuffer_render's and sah_motion_vectors_render's, the G-buffer call's checks first: a
malformed call must answer the status code the header names, a well-formed one gets as far as selecting the device, which a detached
context does not have (SAH_ERR_HIP) — so nothing is ever launched.

    python tests/gbuffer_motion_fuzz_child.py SEED ITERATIONS
"""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib  # noqa: E402
from tests.abi_fuzz_child import Fuzz, _abi_name  # noqa: E402

MAX_EXTENT = 8192
# (field of sah_gbuffer, format, alignment of the address and of the pitch)
TARGETS = (("color", _abi.FORMAT_R8G8B8A8_SRGB, 4), ("normals", _abi.FORMAT_R16G16B16A16_SFLOAT, 8), ("data", _abi.FORMAT_R8G8B8A8_UNORM, 4),
           ("emission", _abi.FORMAT_R8G8B8A8_SRGB, 4), ("depth", _abi.FORMAT_D32_SFLOAT, 4))


def scene_ok(s):
    """sah_gbuffer_render's rule: a scene that draws something brings every array the G-buffer pass reads"""
    if s.num_primitives == 0:
        return True
    return bool(s.primitives and s.indices and s.vertex_positions and s.vertex_data and s.materials) and s.num_materials != 0 and s.num_primitives < (1 << 24)


def plane_ok(p, fmt, w, h, align):
    return (bool(p.ptr) and p.format == fmt and (p.width, p.height) == (w, h) and p.row_pitch_bytes >= w * _abi.FORMAT_BPP[fmt] and p.ptr % align == 0 and
            p.row_pitch_bytes % align == 0)


def expected(ctx, scene, view, out, mv, args):
    if ctx is None or any(a is None for a in args) or not scene_ok(scene):
        return _abi.SAH_ERR_INVALID_ARGUMENT
    w, h = out.depth.width, out.depth.height
    if not (0 < w <= MAX_EXTENT and 0 < h <= MAX_EXTENT):
        return _abi.SAH_ERR_INVALID_ARGUMENT
    if not all(plane_ok(getattr(out, name), fmt, w, h, align) for name, fmt, align in TARGETS):
        return _abi.SAH_ERR_UNSUPPORTED_FORMAT
    if not plane_ok(mv, _abi.FORMAT_R16G16_SFLOAT, w, h, 4):
        return _abi.SAH_ERR_INVALID_ARGUMENT
    return _abi.SAH_ERR_HIP


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
        out = _abi.GBuffer(*[f.plane(fmt, size) for _, fmt, _ in TARGETS])
        mv = f.plane(_abi.FORMAT_R16G16_SFLOAT, size)
        args = [f.ptr(scene), f.ptr(view), f.ptr(out), f.ptr(mv)]
        want = expected(ctx, scene, view, out, mv, args)
        rc = L.sah_gbuffer_motion_render(ctx, *args, f.addr())
        if rc != want:
            planes = "; ".join(f"{name} {p.width}x{p.height} fmt {p.format} pitch {p.row_pitch_bytes} ptr {p.ptr}"
                               for name, p in [(n, getattr(out, n)) for n, _, _ in TARGETS] + [("motion_vectors", mv)])
            print(f"FAIL: sah_gbuffer_motion_render returned {rc}, expected {want} (iteration {i}, seed {seed}): {planes}")
            return 1
        seen[rc] += 1
        f.keep.clear()
    L.sah_destroy(h)
    print("sah_gbuffer_motion_render  " + "  ".join(f"{_abi_name(rc)}: {n}" for rc, n in sorted(seen.items(), reverse=True)))
    if any(seen[rc] == 0 for rc in (_abi.SAH_ERR_HIP, _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT)):
        print("FAIL: the fuzz did not produce every kind of call")
        return 1
    print(f"OK: {iterations} iterations, seed {seed}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
