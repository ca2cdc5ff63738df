"""Rewrites tests/golden/cache_state_trace.json: the traces of tests/test_cache_state_gpu.py's call sequences, recorded from the library that
SAH_HIP_LIBRARY names (default: the one in the tree).  Needs a GPU.

    SAH_HIP_LIBRARY=/path/to/libsah_hip_of_a_commit.so python tools/gen_golden_cache_state.py --commit <hash of that commit>

The fixture is a characterisation: record it from a commit whose behaviour is the one to keep, and name that commit."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="hash of the commit the library was built from (default: HEAD of this checkout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cache_state_trace.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    from tests import test_cache_state_gpu as cs
    traces = {name: cs.record(name).points for name in sorted(cs.SEQUENCES)}
    doc = {"recorded_at_commit": commit, "point": ["label", "cache_epoch", "lpv_copy_rebuilds", "irr32_copy_rebuilds", "table_rebuilt (after sah_lighting)"],
           "traces": traces}
    with open(args.out, "w") as fh:
        fh.write("{\n")
        fh.write(f' "recorded_at_commit": {json.dumps(doc["recorded_at_commit"])},\n "point": {json.dumps(doc["point"])},\n "traces": {{\n')
        for i, (name, points) in enumerate(traces.items()):
            fh.write(f'  {json.dumps(name)}: [\n' + ",\n".join("   " + json.dumps(p) for p in points) + "\n  ]" + ("," if i + 1 < len(traces) else "") + "\n")
        fh.write(" }\n}\n")
    print(f"recorded at commit {commit}: {sum(len(p) for p in traces.values())} points in {len(traces)} sequences -> {args.out}")
    for name, points in traces.items():
        for p in points:
            print(name, p)


if __name__ == "__main__":
    main()
