"""One Lighting case of tests/lighting_cases.py on cuda:0 in a process of its own (run by tests/test_removed_switches_gpu.py, which sets
the environment): the lit image and the dispatch report go into OUT.npz.

    python tests/removed_env_child.py CASE OUT.npz
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from androidrenderer_amd import lib  # noqa: E402
from tests import lighting_cases as lc  # noqa: E402


def main():
    case, out = lc.BY_NAME[sys.argv[1]], sys.argv[2]
    torch.cuda.set_device(0)
    ctx = lib.Context(device=0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        f = case.build()
        lit = f.run_hip(ctx)
        report = ctx.lighting_dispatch()
    finally:
        torch.cuda.synchronize()
        ctx.close()
    np.savez(out, lit=lit, report=np.array(json.dumps(report, sort_keys=True)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
