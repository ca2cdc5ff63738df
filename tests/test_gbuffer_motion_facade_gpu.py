"""GPU: MotionVectorsPhase::share_gbuffer_setup through the C++ host façade (tests/cpp/host_gbuffer_motion.cpp, built by build(); compiled
here when that program is missing).  With the switch on, GbufferPhase::render records the one fused pass (sah_gbuffer_motion_render) and
MotionVectorsPhase::render nothing; with it off — the default — the frame records the two passes it always did.  Both frames are equal,
plane for plane, and equal frame.rasterised_frame with and without `fused_motion`."""
import ctypes as C
import faulthandler
import os
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, mesh
from tests import util
from tests.host_programs import host_program

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = (("color", 4, np.uint8), ("normals", 8, np.uint16), ("data", 4, np.uint8), ("emission", 4, np.uint8), ("depth", 4, np.float32),
          ("motion_vectors", 4, np.uint16))


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)  # an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


def _run_facade(exe, tmp_path, arrays, W, H, share):
    inp, outp = tmp_path / f"in{share}.bin", tmp_path / f"out{share}.bin"
    with open(inp, "wb") as f:
        f.write(np.array([W, H, len(arrays["positions"]), len(arrays["indices"]), len(arrays["primitives"]), len(arrays["materials"])], np.uint32).tobytes())
        for k in ("positions", "vertex_data", "indices", "primitives", "materials"):
            f.write(arrays[k].tobytes())
    stdout = subprocess.run([exe, str(inp), str(outp), str(share)], check=True, timeout=120, capture_output=True, text=True).stdout
    blob = open(outp, "rb").read()
    vd = _abi.ViewData.from_buffer_copy(blob[:C.sizeof(_abi.ViewData)])
    off, out = C.sizeof(_abi.ViewData), {}
    for name, bpp, dtype in PLANES:
        n = W * H * bpp
        out[name] = np.frombuffer(blob[off:off + n], dtype).reshape(H, W, -1)
        off += n
    assert off == len(blob)
    return vd, out, stdout.split()


def test_shared_setup_frame_equals_the_default_frame(tmp_path, hip_ctx):
    import torch
    exe = host_program("host_gbuffer_motion", tmp_path)
    W, H = 320, 180
    arrays = mesh.random_soup(43, triangles=600, extent=8.0).arrays()
    vd_on, on, passes_on = _run_facade(exe, tmp_path, arrays, W, H, 1)
    vd_off, off, passes_off = _run_facade(exe, tmp_path, arrays, W, H, 0)
    assert bytes(vd_on) == bytes(vd_off)
    # one pass ("gbuffer + motion_vectors") against two ("gbuffer", "motion_vectors")
    assert passes_on == ["passes", "1"] and passes_off == ["passes", "2"]
    for name, _, _ in PLANES:
        assert np.array_equal(on[name].view(np.uint8), off[name].view(np.uint8)), name
    assert (on["motion_vectors"] != 0).any() and (on["depth"] > 0).any()
    # the same frame through the Python binding, both ways
    geo = mesh.geometry(mesh.to_device(arrays), [])
    for fused in (False, True):
        planes = {"color": torch.full((H, W, 4), 9, dtype=torch.uint8, device="cuda"), "normals": torch.full((H, W, 4), 9, dtype=torch.int16, device="cuda"),
                  "data": torch.full((H, W, 4), 9, dtype=torch.uint8, device="cuda"), "emission": torch.full((H, W, 4), 9, dtype=torch.uint8, device="cuda"),
                  "depth": torch.full((H, W), 9, dtype=torch.float32, device="cuda")}
        mv = torch.full((H, W, 2), 0x5A5A, dtype=torch.int16, device="cuda")
        frame.rasterised_frame(hip_ctx, geo, vd_on, planes, motion_vectors=mv, fused_motion=fused)
        torch.cuda.synchronize()
        for name, _, dtype in PLANES[:5]:
            assert np.array_equal(util.from_torch(planes[name], dtype).reshape(H, W, -1).view(np.uint8), off[name].view(np.uint8)), (name, fused)
        assert np.array_equal(util.from_torch(mv, np.uint16).reshape(H, W, 2), off["motion_vectors"]), fused
