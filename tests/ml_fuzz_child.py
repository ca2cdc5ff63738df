"""Argument fuzz of the LPV mesh-light entries (include/sah_lpv_mesh_lights.h) in a child process (run by tests/test_lpv_mesh_lights_cpu.py):
NULL arrays, short capacities, indices outside the mesh, unknown flags, bad volume formats and extents, too many entries.  The point cloud
is host code and is fuzzed with real host arrays; the two GPU entries run on a context without a device, so every call that passes the
argument checks ends in a HIP error.  Every call must come back with a sah_status code.

    python tests/ml_fuzz_child.py SEED ITERATIONS
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, lib, mesh  # noqa: E402

STATUS = {_abi.SAH_OK, _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT, _abi.SAH_ERR_HIP, _abi.SAH_ERR_NO_DEVICE, _abi.SAH_ERR_UNSUPPORTED}


def main():
    seed, iterations = int(sys.argv[1]), int(sys.argv[2])
    L = lib.load()
    g = np.random.default_rng(seed)
    arrays = mesh.atrium().arrays()
    pos, vd, idx = arrays["positions"], arrays["vertex_data"], arrays["indices"]
    h = lib.create_detached()
    device_free = h is not None
    pick = lambda *xs: xs[int(g.integers(len(xs)))]
    counts = {}
    for it in range(iterations):
        # the point cloud: real host arrays, made-up ranges, capacities and flags
        n_out = int(pick(0, 1, 5, 64, 70000))
        out_p, out_v = np.zeros((n_out, 3), np.float32), np.zeros(n_out, mesh.VERTEX_DATA)
        count, lo, hi = C.c_uint32(0), (C.c_float * 3)(), (C.c_float * 3)()
        first = int(pick(0, 3, 36, len(idx) - 36, len(idx), len(idx) + 3, 2 ** 32 - 3))
        cnt = int(pick(0, 3, 36, 37, len(idx), 2 ** 32 - 3))
        rc = L.sah_mesh_point_cloud(pick(pos.ctypes.data, None), pick(vd.ctypes.data, None), pick(len(pos), 0, 7), pick(idx.ctypes.data, None), len(idx),
                                    first % 2 ** 32, cnt % 2 ** 32, int(pick(0, -1, 5, -2 ** 31, 2 ** 31 - 1)), int(g.integers(2 ** 63)), int(pick(0, 1, 2, 0xFFFFFFFF)),
                                    pick(out_p.ctypes.data if n_out else None, None), pick(out_v.ctypes.data if n_out else None, None),
                                    pick(n_out, 0, 2 ** 32 - 1) if n_out else pick(0, 1), pick(C.byref(count), None), pick(lo, None), pick(hi, None))
        assert rc in STATUS, ("sah_mesh_point_cloud", rc)
        counts[rc] = counts.get(rc, 0) + 1
        if not device_free:
            continue
        ctx = pick(h, h, h, None)
        geom = mesh.geometry(mesh.with_counts(arrays)) if g.random() < 0.9 else None
        vols = (_abi.Volume * 3)(*[_abi.Volume(0x1000 * (1 + c), int(pick(128, 128, 129, 4096)), 32, int(pick(32, 32, 33)), int(pick(1024, 1028, 8)),
                                               32 * 1024, int(pick(_abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_R16G16B16A16_SFLOAT, 43)))
                                   for c in range(3)])
        rc = L.sah_lpv_emissive_vpls(ctx, C.byref(geom) if geom is not None else None, int(pick(0, 9, 31, 32, 2 ** 32 - 1)), pick(0x1000, None),
                                     pick(0x2000, None), int(pick(0, 5, 65536)), int(pick(0, 1, 2)), pick(0x3000, None))
        assert rc in STATUS, ("sah_lpv_emissive_vpls", rc)
        n = int(pick(0, 1, 8, 40))
        clouds = (lib.EmissiveCloud * max(n, 1))(*[lib.EmissiveCloud(pick(0x4000, None), int(pick(0, 5, 65536, 2 ** 24, 2 ** 32 - 1)), int(pick(9, 0, 99)))
                                                   for _ in range(n)])
        mats, bounds = (_abi.LpvCascadeMatrices * 4)(), (lib.LpvCascadeBounds * 4)()
        rc = L.sah_lpv_inject_emissive(ctx, C.byref(geom) if geom is not None else None, pick(clouds, None), n, pick(mats, None), pick(bounds, None),
                                       int(pick(0, 1, 4, 5, 2 ** 32 - 1)), pick(vols, None))
        assert rc in STATUS, ("sah_lpv_inject_emissive", rc)
    if device_free:
        L.sah_destroy(h)
    print(f"OK: {iterations} iterations", counts)
    return 0


if __name__ == "__main__":
    sys.exit(main())
