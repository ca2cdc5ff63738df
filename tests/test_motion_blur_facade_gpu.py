"""GPU: frames of sah_motion_blur through the C++ host façade's MotionBlurPhase (tests/cpp/host_motion_blur, in a child process) against the
Python path and the numpy restatement, bit for bit.  The façade's own SceneView carries z_near and the two jitters, and its view block comes
back with each plane; the second frame's previous jitter is the first frame's; the third renders below its output extent, so the phase
re-creates its textures."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import _abi
from tests import motion_blur_ref as ref
from tests.test_motion_blur_gpu import Planes, _params
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
    # (output extent, render extent, dither, sample count, view jitter, shutter)
    frames = [((80, 36), (80, 36), 0, 12, (0.25, -0.125), 0.5), ((80, 36), (80, 36), 1, 32, (-0.375, 0.125), 1.0), ((60, 50), (40, 33), 1, 6, (0.125, 0.375), 0.5)]
    arrays = []
    for i, ((W, H), (w, h), *_) in enumerate(frames):
        g = np.random.default_rng(500 + i)
        depth = ref.box_depth(w, h)
        mv = ref.to_half_bits(np.where(ref.box_mask(w, h)[..., None], np.array([17.0, -8.0]), np.array([-3.0, 2.0])) + g.normal(0.0, 0.05, (h, w, 2)))
        arrays.append((ref.textured_scene(W, H, 500 + i), depth, mv))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(frames)], np.uint32).tobytes())
        for ((W, H), (w, h), dither, count, jitter, shutter), planes in zip(frames, arrays):
            f.write(np.array([W, H, w, h, dither, count], np.uint32).tobytes() + np.array(list(jitter) + [shutter], f32).tobytes())
            for a in planes:
                f.write(np.ascontiguousarray(a).tobytes())
    subprocess.check_call([host_program("host_motion_blur", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    at, previous, blurred = 0, (0.0, 0.0), 0
    for i, (((W, H), (w, h), dither, count, jitter, shutter), (scene_bits, depth, mv)) in enumerate(zip(frames, arrays)):
        view = _abi.ViewData.from_buffer_copy(blob[at:at + 432])
        facade = np.frombuffer(blob[at + 432:at + 432 + W * H * 8], np.uint16).reshape(H, W, 4)
        at += 432 + W * H * 8
        assert tuple(view.render_resolution) == (w, h) and tuple(view.jitter) == tuple(f32(j) for j in jitter)
        assert tuple(view.previous_jitter) == tuple(f32(j) for j in previous) and f32(view.z_near) == f32(0.05)
        settings = dict(shutter=shutter, sample_count=count, flags=ref.DITHER if dither else 0, z_near=0.05, jitter=jitter, previous_jitter=previous)
        want, info = ref.motion_blur_ex(scene_bits, depth, mv, **settings)
        assert same(facade, want), f"frame {i}: " + differs(facade, want)
        got = Planes(scene_bits, depth, mv).run(hip_ctx, _params(**settings))
        assert same(facade, got)
        blurred += int((~info["passed"]).sum())
        previous = jitter
    assert at == len(blob) and blurred > 3000
