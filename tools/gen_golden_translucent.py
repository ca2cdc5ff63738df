"""Writes tests/golden/translucent_96x54.npz: the composition of tests/translucent_ref.py on the CPU oracle's rasteriser and lighting.

    python tools/gen_golden_translucent.py

96 x 54 is two 64 x 64 tiles, both partial.  The scene is translucent_ref.scene_panes(): the atrium with seven translucent primitives in it
— over the sky, behind opaque geometry, textured with random vertex colours, emissive, metallic, back-facing —, lit by the cascaded sun and
the LPV.  The fixture holds the opaque depth plane, the lit image before the pass (`lit0`), the image after it (`lit`) and, per pixel, how
many fragments were blended."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from androidrenderer_amd import _abi  # noqa: E402
from tests import translucent_ref as ref  # noqa: E402

WIDTH, HEIGHT = 96, 54
FIXTURE = os.path.join(ROOT, "tests", "golden", f"translucent_{WIDTH}x{HEIGHT}.npz")
SUN, GI = _abi.SHADOW_MODE_CSM, _abi.GI_LPV


def frame(backend):
    return ref.Frame(backend, ref.scene_panes(), WIDTH, HEIGHT, SUN, GI)


def generate():
    fr = frame(ref.OracleBackend())
    lit, blended = fr.compose()
    ref.assert_preconditions(fr, lit, blended, min_changed=0.2, min_depth=3)
    return {"depth": fr.depth, "lit0": np.array(fr.lit0), "lit": lit, "blended": blended.astype(np.uint8)}


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(FIXTURE, **data)
    changed = (data["lit"] != data["lit0"]).any(-1)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; {float(changed.mean()):.2f} of the pixels change, the deepest blends {int(data['blended'].max())} fragments")
