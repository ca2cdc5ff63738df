"""GPU: frames of sah_ssr through the C++ host façade's ScreenSpaceReflections (tests/cpp/host_ssr, in a child process) against the Python
path and the numpy restatement, bit for bit.  The façade's own SceneView forms the view block, which comes back with each plane; the second
frame takes a copy of the first's output as its source; the third has another extent, so the phase re-creates its textures."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import _abi
from tests import ssr_ref as ref
from tests.test_ssr_gpu import INPUTS, Planes, _params
from tests.host_programs import host_program
from tests.support import differs, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def test_three_frames_through_the_cpp_facade(tmp_path, hip_ctx):
    # (width, height, source is the previous output, jitter flag, reflection only, view jitter, stride, thickness)
    frames = [(80, 36, 0, 0, 0, (0.25, -0.125), 4.0, 0.5), (80, 36, 1, 1, 0, (-0.375, 0.125), 2.5, 3e38), (45, 50, 0, 0, 1, (0.125, 0.375), 1.0, 0.5)]
    arrays = [ref.random_frame(w, h, 400 + i) for i, (w, h, *_) in enumerate(frames)]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(frames)], np.uint32).tobytes())
        for (w, h, prev, jit, only, jitter, stride, thick), a in zip(frames, arrays):
            f.write(np.array([w, h, prev, jit, only], np.uint32).tobytes() + np.array(list(jitter) + [stride, thick], f32).tobytes())
            for k in ("color", "normals", "data", "depth", "lit"):
                f.write(np.ascontiguousarray(a[k]).tobytes())
    subprocess.check_call([host_program("host_ssr", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    at, previous, hits = 0, None, 0
    for i, ((w, h, prev, jit, only, jitter, stride, thick), a) in enumerate(zip(frames, arrays)):
        view = _abi.ViewData.from_buffer_copy(blob[at:at + 432])
        facade = np.frombuffer(blob[at + 432:at + 432 + w * h * 8], np.uint16).reshape(h, w, 4)
        at += 432 + w * h * 8
        assert tuple(view.render_resolution) == (w, h) and tuple(view.jitter) == tuple(f32(j) for j in jitter) and view.projection[8] != 0
        settings = dict(stride_pixels=stride, thickness=thick, flags=(ref.JITTER if jit else 0) | (ref.REFLECTION_ONLY if only else 0))
        inputs = dict({k: a[k] for k in INPUTS}, source=previous if prev else a["lit"])
        want, info = ref.ssr_ex(view=ref.View(view), params=settings, **inputs)
        assert same(facade, want), f"frame {i}: " + differs(facade, want)
        got = Planes(inputs).run(hip_ctx, view, _params(**settings))
        assert same(facade, got)
        hits += int(info["hit"].sum())
        previous = facade
    assert at == len(blob) and hits > 300
