"""GPU: RaytracingScene::update_primitive through the C++ host façade (tests/cpp/host_rt_refit.cpp, built by build(); compiled here when
that program is missing): two traced frames with one primitive moved in between.  A façade that refits ("Refit TLAS", sah_rt_refit) and
one that rebuilds ("Build TLAS") must print the same AO and shadow-mask hashes for both frames."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import mesh, synth
from tests import rt_structure_scenes as scenes
from tests.host_programs import host_program

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)  # an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


def test_a_moved_primitive_through_the_cpp_facade(tmp_path):
    W, H, moving = 96, 54, 0  # the atrium's primitive 0 is its floor: seen from the start-up camera whichever way it looks
    arrays = mesh.atrium(2).arrays()
    assert moving < len(arrays["primitives"])
    model = scenes.rotation_y(0.5, (0.6, 0.4, -0.8))
    noise = synth.rng(21).integers(0, 256, (128, 128, 4), dtype=np.uint8)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([W, H, len(arrays["positions"]), len(arrays["indices"]), len(arrays["primitives"]), len(arrays["materials"]), moving], np.uint32).tobytes())
        for k in ("positions", "vertex_data", "indices", "primitives", "materials"):
            f.write(np.ascontiguousarray(arrays[k]).tobytes())
        f.write(noise.tobytes())
        f.write(np.ascontiguousarray(model, np.float32).tobytes())
    exe = host_program("host_rt_refit", tmp_path)
    out = {mode: subprocess.run([exe, str(inp), mode], check=True, timeout=120, capture_output=True, text=True).stdout.splitlines() for mode in ("refit", "rebuild")}
    assert len(out["refit"]) == len(out["rebuild"]) == 2
    assert out["refit"][0] == out["rebuild"][0] and out["refit"][0].startswith("frame 0 Build TLAS depth ")
    assert out["refit"][1].startswith("frame 1 Refit TLAS depth ") and out["rebuild"][1].startswith("frame 1 Build TLAS depth ")
    assert out["refit"][1].split(" depth ")[1] == out["rebuild"][1].split(" depth ")[1], (out["refit"][1], out["rebuild"][1])
    first, second = (dict(zip(line.split()[4::2], line.split()[5::2])) for line in out["refit"])
    assert set(first) == {"depth", "ao", "mask"}
    assert all(first[k] != second[k] for k in first), "the moved primitive changed nothing: the frames compare nothing"
