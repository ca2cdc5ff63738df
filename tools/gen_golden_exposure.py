"""Writes tests/golden/exposure_69x21.npz with the numpy restatement of sah_exposure_meter / sah_exposure_apply (tests/exposure_ref.py).

    python tools/gen_golden_exposure.py

69 x 21 is a multiple of neither dimension of the kernel's 128 x 4 tile, and odd: every row ends on the single-pixel tail of a two-pixel
lane.  The scene is stored with the padded pitch it was generated with (70 texels), the padding holding a pattern no texel has.  It is a
log-normal image 2.5 octaves wide with the uncounted pixels (zeros, -0, negatives, NaN, +-inf), half denormals and luminances beyond both
ends of the histogram that exposure_ref.random_inputs plants.  Three frames follow one another with adaptation 0.25: frame i is the scene
multiplied by GAINS[i] (restated: exposure_ref.apply), the first is metered with SAH_EXPOSURE_HISTORY_INVALID and exposed by its own state
(meter, then apply), the next two take the fused form and are exposed by the state of the frame before."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import exposure_ref as ref  # noqa: E402

WIDTH, HEIGHT = 69, 21
PITCH = 70  # in texels
FIXTURE = os.path.join(ROOT, "tests", "golden", f"exposure_{WIDTH}x{HEIGHT}.npz")
PARAMS = dict(key=0.18, low_fraction=0.5, high_fraction=0.95, min_exposure=1.0 / 64.0, max_exposure=64.0, adaptation=0.25)
GAINS = (1.0, 8.0, 0.125)


def frames(scene):
    """the three frames' scenes"""
    return [ref.apply(scene, g) for g in GAINS]


def sequence(scenes, settings, fused_from=1):
    """[(histogram, state, exposed)] of successive frames: the first with HISTORY_INVALID, metered and then exposed by its own state; the
    others fused — exposed by the state of the frame before"""
    out, state = [], None
    for i, sc in enumerate(scenes):
        first = i < fused_from
        n, new = ref.meter(sc, None if first else state, dict(settings, flags=ref.HISTORY_INVALID if first else 0))
        out.append((n, new, ref.apply(sc, new["exposure"] if first else state["exposure"])))
        state = new
    return out


def generate(seed):
    scene = ref.random_inputs(WIDTH, HEIGHT, seed)
    plane = np.full((HEIGHT, PITCH, 4), np.uint16(0xA5A5))
    plane[:, :WIDTH] = scene
    seq = sequence(frames(scene), PARAMS)
    return {"seed": np.int64(seed), "width": np.int64(WIDTH), "scene_plane": plane, "gains": np.array(GAINS, np.float32),
            "params": np.array([PARAMS[k] for k in sorted(PARAMS)], np.float32), "histograms": np.stack([n for n, _, _ in seq]),
            "states": np.stack([s for _, s, _ in seq]), "exposed": np.stack([e for _, _, e in seq])}


if __name__ == "__main__":
    data = generate(6921)
    np.savez_compressed(FIXTURE, **data)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; states {data['states'].tolist()}; bins in use {int((data['histograms'][0] > 0).sum())}")
