"""GPU: LPV mesh lights through the C++ host façade (tests/cpp/host_lpv_mesh_lights.cpp, compiled here): with mesh_lights on,
inject_indirect_sun_light ends with the emissive injection and its volumes equal the sun chain's plus the direct ABI calls
(mesh.emissive_clouds + sah_lpv_inject_emissive) bit for bit; with it off the recorded passes are today's; the injection alone equals the
direct calls onto cleared volumes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import _abi, images, lib, mesh
from tests import util
from tests.host_programs import host_program

pytestmark = pytest.mark.gpu
SHAPE = (32, 32, 128, 4)


def test_mesh_lights_through_cpp_facade(tmp_path, hip_ctx):
    import torch
    exe = host_program("host_lpv_mesh_lights", tmp_path)  # (not among those build() leaves: compiled here)
    arrays = mesh.atrium().arrays()
    arrays["textures"], arrays["material_textures"] = [], np.zeros((0, 4), np.uint32)
    seed, flags = 77, lib.POINT_CLOUD_ON_SURFACE
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(arrays["positions"]), len(arrays["indices"]), len(arrays["primitives"]), len(arrays["materials"]), seed, flags],
                         np.uint32).tobytes())
        for k in ("positions", "vertex_data", "indices", "primitives", "materials"):
            f.write(np.ascontiguousarray(arrays[k]).tobytes())
    subprocess.check_call([exe, str(inp), str(outp)], timeout=300)
    blob = open(outp, "rb").read()
    off = 0

    def take(n):
        nonlocal off
        off += n
        return blob[off - n:off]
    n_clouds = int(np.frombuffer(take(4), np.uint32)[0])
    mats = (_abi.LpvCascadeMatrices * 4).from_buffer_copy(take(4 * C.sizeof(_abi.LpvCascadeMatrices)))
    bounds = (lib.LpvCascadeBounds * 4).from_buffer_copy(take(4 * C.sizeof(lib.LpvCascadeBounds)))
    frames = []
    for _ in range(3):
        passes = int(np.frombuffer(take(4), np.uint32)[0])
        frames.append((passes, [np.frombuffer(take(128 * 32 * 32 * 8), np.uint16).reshape(SHAPE) for _ in range(3)]))
    assert n_clouds == len(mesh.emissive_primitives(arrays)) == 8
    assert frames[0][0] == 5 and frames[1][0] == 6 and frames[2][0] == 1  # Render RSM + 4 x extract / inject (+ the emissive injection)
    g = mesh.geometry(mesh.to_device(arrays), [])
    records, keep = mesh.emissive_clouds(hip_ctx, arrays, g, seed, flags)
    for prior, want_frame in ((np.zeros(SHAPE, np.uint16), 2), (None, 1)):
        vols = [util.to_torch((prior if prior is not None else frames[0][1][c]).copy()) for c in range(3)]
        hip_ctx.lpv_inject_emissive(g, records, mats, bounds, 4, [images.volume(t, _abi.FORMAT_R16G16B16A16_SFLOAT) for t in vols])
        torch.cuda.synchronize()
        for c in range(3):
            got = util.from_torch(vols[c], np.uint16).reshape(SHAPE)
            assert np.array_equal(got, frames[want_frame][1][c]), (want_frame, c)
    assert np.count_nonzero(frames[2][1][0]) and not np.array_equal(frames[0][1][0], frames[1][1][0])
