"""GPU: the C++ host façade's DepthCullingPhase and MipChainGenerator (tests/cpp/host_hi_z.cpp, built by build(); compiled here when that
program is missing): the Hi-Z pyramid of a rasterised 160 x 96 G-buffer depth plane, against the numpy restatement and the direct call."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import _abi, images, mesh, scene
from tests import mip_chain_ref as ref
from tests.host_programs import host_program

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)  # an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


def test_hi_z_of_a_rasterised_depth_plane_through_cpp_facade(tmp_path, hip_ctx):
    import torch
    W, H = 160, 96
    arrays = mesh.random_soup(43, triangles=400, extent=8.0).arrays()
    view = scene.SceneView.default(W, H)
    keep = []
    geo = mesh.geometry(mesh.to_device(arrays), keep)
    gb = {"color": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), "normals": torch.zeros((H, W, 4), dtype=torch.int16, device="cuda"),
          "data": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), "emission": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"),
          "depth": torch.zeros((H, W), dtype=torch.float32, device="cuda")}
    hip_ctx.gbuffer_render(geo, view.gpu_data, images.gbuffer(gb))
    torch.cuda.synchronize()
    depth = gb["depth"].cpu().numpy()
    assert (depth > 0).any() and len(np.unique(depth)) > 1000  # geometry, not a constant plane
    extent0, n = ref.hi_z_extent_and_levels((W, H))
    assert extent0 == (80, 48) and n == 6 and ref.spd_mips(W, H) == 7  # one level is missing: the stray store is part of the result
    want = ref.generate(depth, ref.FORMAT_D32, extent0, n)
    # through the façade
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([W, H], np.uint32).tobytes())
        f.write(depth.tobytes())
    subprocess.check_call([host_program("host_hi_z", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    assert int(np.frombuffer(blob[:4], np.uint32)[0]) == n
    at = 4
    for i in range(n):
        w, h = (int(v) for v in np.frombuffer(blob[at:at + 8], np.uint32))
        assert (w, h) == ref.level_extents(extent0, n)[i]
        level = np.frombuffer(blob[at + 8:at + 8 + w * h * 4], np.uint32).reshape(h, w)
        at += 8 + w * h * 4
        assert np.array_equal(level, want[i]), f"level {i}: {int((level != want[i]).sum())} texels differ"
    assert at == len(blob)
    # the direct call
    levels_t = [torch.zeros((h, w), dtype=torch.float32, device="cuda") for w, h in ref.level_extents(extent0, n)]
    hip_ctx.mip_chain_generate(images.plane(gb["depth"], _abi.FORMAT_D32_SFLOAT), [images.plane(t, _abi.FORMAT_R32_SFLOAT) for t in levels_t])
    torch.cuda.synchronize()
    for i, t in enumerate(levels_t):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), want[i]), i
    assert want[1][0, 0] != ref.generate(depth, ref.FORMAT_D32, extent0, 7)[1][0, 0] or want[1][0, 0] == 0
