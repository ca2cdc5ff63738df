"""GPU: the library launches what its arguments say, whatever the environment holds.  The experiment switches the library once read with
getenv (tools/experiments/r6/README.md lists them) are gone: with every one of them set, a Lighting case with a sky and an LPV gives the
same image and the same dispatch report as without them.  Each run is a fresh child process (the library read some of them once per
process), bounded in time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lighting_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REMOVED = {"SAH_SKY_INTERLEAVED": "1", "SAH_SKY_RATIO": "7", "SAH_TILED_GENERAL_GEOMETRY": "1", "SAH_TILED_GENERAL_LPV": "1", "SAH_FORCE_PPT": "1",
           "SAH_FORCE_GENERAL": "1", "SAH_LPV_MODE": "3", "SAH_LPV_GV_MODE": "2", "SAH_TM_THREADS": "512", "SAH_TM_BAND16": "1"}
CASE = "sky-sky_trailing_rows-lpv"  # sky bound, RT sun, LPV overlay: the fast kernel with its leading sky workgroups


def _run(tmp_path, tag, extra):
    env = {k: v for k, v in os.environ.items() if k not in REMOVED}
    env.update(extra)
    out = tmp_path / f"{tag}.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "removed_env_child.py"), CASE, str(out)], env=env, timeout=300)
    assert p.returncode == 0, f"{tag}: the child ended with {p.returncode}"
    z = np.load(out)
    return z["lit"], json.loads(str(z["report"]))


def test_removed_switches_change_nothing(tmp_path):
    lit0, rep0 = _run(tmp_path, "clean", {})
    lit1, rep1 = _run(tmp_path, "set", REMOVED)
    print(f"{CASE}: clean {rep0}\n{CASE}: with the removed variables set {rep1}")
    case = lc.BY_NAME[CASE]
    for k, v in case.expect.items():
        assert rep0[k] == v, f"{CASE}: {k} = {rep0[k]}, the case expects {v}"
    assert rep0["family"] == "fast" and rep0["sky_workgroups"] > 0, rep0  # (the case does run what the sky switches used to reorder)
    assert rep1 == rep0, "the dispatch report depends on a removed environment variable"
    assert np.array_equal(lit1, lit0), "the lit image depends on a removed environment variable"
