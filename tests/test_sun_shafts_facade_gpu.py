"""GPU: frames of sah_sun_shafts through the C++ host façade's SunShafts (tests/cpp/host_sun_shafts, in a child process) against the Python
path and the numpy restatement, bit for bit on the output and on the march plane.  The façade's own SceneView and DirectionalLight form the
view block and the cascades, which come back with each frame, as does the step transmittance the façade made of the extinction; the dither
offset steps per frame; the third frame has another extent and downscale, so the object re-creates its textures; the last has no map."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import _abi
from tests import sun_shafts_ref as ref
from tests.test_sun_shafts_gpu import Map, Planes, _params, _same
from tests.host_programs import host_program
from tests.support import differs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def test_four_frames_through_the_cpp_facade(tmp_path, hip_ctx):
    # (extent, downscale, dither, steps, map resolution, layers, D32, extinction, step length, ambient)
    frames = [((80, 36), 1, 0, 32, 64, 4, 0, 0.04, 0.5, 0.0), ((80, 36), 1, 1, 24, 32, 3, 1, 0.1, 0.4, 1e-5), ((47, 33), 2, 1, 16, 16, 2, 0, 0.02, 1.0, 2e-5),
              ((47, 33), 2, 1, 8, 0, 0, 0, 0.3, 2.0, 0.0)]
    arrays = []
    for i, ((w, h), _, _, _, res, layers, d32, *_) in enumerate(frames):
        shadow = ref.noise_map(layers, res, 600 + i, f32 if d32 else np.uint16, block=4) if layers else None
        arrays.append((ref.box_depth(w, h, seed=i), ref.textured_lit(w, h, 500 + i), shadow))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(frames)], np.uint32).tobytes())
        for ((w, h), s, dither, steps, res, layers, d32, extinction, step_length, ambient), planes in zip(frames, arrays):
            f.write(np.array([w, h, s, dither, steps, res, layers, d32], np.uint32).tobytes() + np.array([extinction, step_length, ambient], f32).tobytes())
            for a in planes:
                if a is not None:
                    f.write(np.ascontiguousarray(a).tobytes())
    subprocess.check_call([host_program("host_sun_shafts", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    at, changed, taps = 0, 0, 0
    for i, (((w, h), s, dither, steps, res, layers, d32, extinction, step_length, ambient), (depth, lit, shadow)) in enumerate(zip(frames, arrays)):
        view = _abi.ViewData.from_buffer_copy(blob[at:at + 432])
        sun = _abi.SunLightConstants.from_buffer_copy(blob[at + 432:at + 432 + 640])
        tau = np.frombuffer(blob[at + 1072:at + 1076], f32)[0]
        at += 1076
        mw, mh = (w + s - 1) // s, (h + s - 1) // s
        facade = np.frombuffer(blob[at:at + w * h * 8], np.uint16).reshape(h, w, 4)
        march = np.frombuffer(blob[at + w * h * 8:at + w * h * 8 + mw * mh * 8], np.uint16).reshape(mh, mw, 4)
        at += w * h * 8 + mw * mh * 8
        assert tuple(view.render_resolution) == (w, h) and f32(view.z_near) == f32(0.05) and sun.shadow_mode == _abi.SHADOW_MODE_CSM
        assert abs(float(tau) - np.exp(-float(f32(extinction)) * float(f32(step_length)))) < 1e-6  # the façade's exponential, to fp32
        settings = dict(step_length=step_length, num_steps=steps, step_transmittance=float(tau), albedo=(_abi.LIGHTING_EXPOSURE,) * 3, ambient=(ambient,) * 3,
                        downscale=s, dither_offset=i & 15 if dither else 0, flags=ref.DITHER if dither else 0)  # (the pass without planes took no offset)
        want, info = ref.sun_shafts_ex(view, sun, shadow, depth, lit, **settings)
        assert _same(march, info["bits"]), f"frame {i}: march " + differs(march, info["bits"])
        assert _same(facade, want), f"frame {i}: " + differs(facade, want)
        got = Planes(depth, lit, s).run(hip_ctx, dict(view=view, sun=sun), None if shadow is None else Map(shadow), _params(**settings))
        assert _same(facade, got)
        changed += int((want != lit).any(-1).sum())
        taps += info["taps"]
    assert at == len(blob) and changed > 5000 and taps > 5000
