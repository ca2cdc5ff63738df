"""GPU: the C++ host façade's MotionVectorsPhase (tests/cpp/host_motion_vectors.cpp, compiled here) and frame.rasterised_frame.  With
`needs_motion_vectors` on, the façade's target equals the C call bit for bit; with it off — the default — no pass is added, the target
stays as it was created and the G-buffer planes are the ones the frame writes without the feature."""
import ctypes as C
import faulthandler
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, images, mesh
from tests import util
from tests.host_programs import host_program

pytestmark = pytest.mark.gpu
PLANES = (("color", 4, np.uint8), ("normals", 8, np.uint16), ("data", 4, np.uint8), ("emission", 4, np.uint8), ("depth", 4, np.float32),
          ("motion_vectors", 4, np.uint16))


def _run_facade(exe, tmp_path, arrays, W, H, switch):
    inp, outp = tmp_path / f"in{switch}.bin", tmp_path / f"out{switch}.bin"
    with open(inp, "wb") as f:
        f.write(np.array([W, H, len(arrays["positions"]), len(arrays["indices"]), len(arrays["primitives"]), len(arrays["materials"])], np.uint32).tobytes())
        for k in ("positions", "vertex_data", "indices", "primitives", "materials"):
            f.write(arrays[k].tobytes())
    subprocess.check_call([exe, str(inp), str(outp), str(switch)], timeout=300)
    blob = open(outp, "rb").read()
    vd = _abi.ViewData.from_buffer_copy(blob[:C.sizeof(_abi.ViewData)])
    off, out = C.sizeof(_abi.ViewData), {}
    for name, bpp, dtype in PLANES:
        n = W * H * bpp
        out[name] = np.frombuffer(blob[off:off + n], dtype).reshape(H, W, -1)
        off += n
    assert off == len(blob)
    return vd, out


def test_motion_vectors_phase_through_cpp_facade(tmp_path, hip_ctx):
    import torch
    exe = host_program("host_motion_vectors", tmp_path)  # (not among those build() leaves: compiled here)
    W, H = 320, 180
    arrays = mesh.random_soup(43, triangles=600, extent=8.0).arrays()
    vd_on, on = _run_facade(exe, tmp_path, arrays, W, H, 1)
    vd_off, off = _run_facade(exe, tmp_path, arrays, W, H, 0)
    assert bytes(vd_on) == bytes(vd_off)
    # the switch off: no motion vectors (the target is as created), and the frame's planes do not depend on the switch
    assert (off["motion_vectors"] == 0).all()
    for name, _, _ in PLANES[:5]:
        assert np.array_equal(on[name], off[name]), name
    # the same frame through the Python binding: G-buffer, then the opt-in motion-vectors target
    keep = []
    geo = mesh.geometry(mesh.to_device(arrays), keep)

    def targets():
        return {"color": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), "normals": torch.zeros((H, W, 4), dtype=torch.int16, device="cuda"),
                "data": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), "emission": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"),
                "depth": torch.zeros((H, W), dtype=torch.float32, device="cuda")}
    plain, with_mv = targets(), targets()
    mv = torch.zeros((H, W, 2), dtype=torch.int16, device="cuda")
    for kwargs, planes in (({}, plain), ({"motion_vectors": mv}, with_mv)):
        faulthandler.dump_traceback_later(120, exit=True)  # each GPU step under a limit of its own: an overrun ends the process
        try:
            frame.rasterised_frame(hip_ctx, geo, vd_on, planes, **kwargs)
            torch.cuda.synchronize()
        finally:
            faulthandler.cancel_dump_traceback_later()
    for name, _, dtype in PLANES[:5]:
        a = util.from_torch(plain[name], dtype).reshape(H, W, -1)
        assert np.array_equal(a, util.from_torch(with_mv[name], dtype).reshape(H, W, -1)), name
        assert np.array_equal(a.view(np.uint8), off[name].view(np.uint8)), name  # the façade's default frame is the binding's
    got = util.from_torch(mv, np.uint16).reshape(H, W, 2)
    assert (got != 0).any()
    g16, w16 = got.view(np.float16), on["motion_vectors"].view(np.float16)
    assert np.array_equal(np.isnan(g16), np.isnan(w16)) and np.array_equal(got[~np.isnan(g16)], on["motion_vectors"][~np.isnan(w16)])
