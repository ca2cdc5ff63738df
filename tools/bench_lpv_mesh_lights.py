"""Timings of the LPV mesh lights (include/sah_lpv_mesh_lights.h) on cuda:0, from HIP events around N back-to-back calls (after a warm-up):

    python tools/bench_lpv_mesh_lights.py [--calls 200]

  atrium_4c        sah_lpv_inject_emissive, the atrium's 8 lamps (on-surface clouds), 4 cascades: 160 entries, the single-workgroup form
  synth_256k       ... 5 clouds of random lights around the camera, 256 Ki entries (points x 4 cascades)
  synth_1m         ... 1 Mi entries
  synth_4m         ... 4 Mi entries
  hot_cell_1m      ... 1 Mi entries of which every light lies on one position: one cell per cascade takes 65,536 serial adds
  vpls_64k         sah_lpv_emissive_vpls of a 65,536-point cloud with a trilinear emission texture

Prints one JSON line, milliseconds per call, with the ratio synth_4m / synth_1m (no quadratic term: <= 5 expected)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, images, lib, mesh
    from tests import util
    from tests.test_lpv_mesh_lights_gpu import _lpv, _synthetic

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    vol = lambda t: images.volume(t, _abi.FORMAT_R16G16B16A16_SFLOAT)
    A = [torch.zeros((32, 32, 128, 4), dtype=torch.int16, device="cuda") for _ in range(3)]
    AV = [vol(t) for t in A]
    keep = []

    arrays = mesh.atrium().arrays()
    view, sun, lpv = _lpv(1920, 1080)
    g_atrium = mesh.geometry(mesh.to_device(arrays), keep)
    atrium, k = mesh.emissive_clouds(ctx, arrays, g_atrium, 1, lib.POINT_CLOUD_ON_SURFACE)
    keep.append(k)

    def synth(entries, hot):
        points = entries // 4 // 4
        s_arrays, s_lpv, vp, lo, hi = _synthetic(4, points, points if hot else 0, 5)
        if hot:
            for v in vp[1:]:
                v[:, :2] = vp[0][0, :2]
        g = mesh.geometry(mesh.to_device(s_arrays), keep)
        ts = [util.to_torch(np.ascontiguousarray(v)) for v in vp]
        keep.append(ts)
        recs = [lib.EmissiveCloud(t.data_ptr(), len(v), i, (C.c_float * 3)(*lo.tolist()), (C.c_float * 3)(*hi.tolist())) for i, (t, v) in enumerate(zip(ts, vp))]
        return lambda: ctx.lpv_inject_emissive(g, recs, s_lpv.matrices, s_lpv.bounds, 4, AV)

    m = mesh.Mesh()
    rng = np.random.default_rng(3)
    tex = m.add_texture(*mesh.random_texture(rng, 256, 256, None, True, mesh.sampler(bias=0.5)))
    mat = m.add_material(mesh.material(emission=(2.0, 1.0, 0.5, 0.0)), emission=tex)
    m.add_primitive([[0, 0, 0], [200, 0, 0], [0, 200, 0]], [[0, 0, 1]] * 3, [0, 1, 2], mat, texcoords=[[0, 0], [1, 0], [0, 1]])
    big = m.arrays()
    g_big = mesh.geometry(mesh.to_device(big), keep)
    pos, pts, _, _ = lib.mesh_point_cloud(big["positions"], big["vertex_data"], big["indices"], 0, 3, 0, 9, lib.POINT_CLOUD_ON_SURFACE)
    assert len(pos) == 65536
    pos_t, pts_t = util.to_torch(pos), util.to_torch(pts.view(np.uint8).reshape(-1))
    out_t = torch.zeros((65536, 4), dtype=torch.int32, device="cuda")

    cases = {
        "atrium_4c": lambda: ctx.lpv_inject_emissive(g_atrium, atrium, lpv.matrices, lpv.bounds, 4, AV),
        "synth_256k": synth(1 << 18, False),
        "synth_1m": synth(1 << 20, False),
        "synth_4m": synth(1 << 22, False),
        "hot_cell_1m": synth(1 << 20, True),
        "vpls_64k": lambda: ctx.lpv_emissive_vpls(g_big, 0, pos_t.data_ptr(), pts_t.data_ptr(), 65536, 0, out_t.data_ptr()),
    }
    out = {"calls": args.calls, "unit": "ms per call", "atrium_entries": sum(r.count for r in atrium) * 4}
    for name, fn in cases.items():
        calls = args.calls if not name.startswith(("synth_4m", "hot")) else max(args.calls // 4, 1)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = round(e0.elapsed_time(e1) / calls, 5)
    out["ratio_4m_over_1m"] = round(out["synth_4m"] / out["synth_1m"], 3)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
