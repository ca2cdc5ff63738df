"""Print per-kernel register/LDS/occupancy usage for a HIP source (hipcc -Rpass-analysis=kernel-resource-usage) and each kernel's code
length in bytes (the size of its symbol in the device object), compiled with the library's options (androidrenderer_amd/build.py: FLAGS and the per-source SOURCE_FLAGS of the file's name).

    python tools/kernel_resources.py androidrenderer_amd/csrc/lighting.hip"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import build as hip_build  # noqa: E402

import tempfile

src = sys.argv[1]
# (the device half alone, into an object that is kept for a moment: its symbol table has each kernel's code length)
with tempfile.TemporaryDirectory() as tmp:
    obj = os.path.join(tmp, "device.o")
    cmd = (["/opt/rocm/bin/hipcc"] + hip_build.FLAGS + hip_build.SOURCE_FLAGS.get(os.path.basename(src), []) +
           ["--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj, "-Rpass-analysis=kernel-resource-usage"])
    out = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.PIPE, text=True).stderr
    code_bytes = {}
    if os.path.exists(obj):
        syms = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-s", "--wide", obj], stdout=subprocess.PIPE, text=True).stdout
        for line in syms.splitlines():
            f = line.split()
            if len(f) == 8 and f[3] == "FUNC":
                code_bytes[f[7]] = int(f[2], 0)
rows, cur = [], {}
for line in out.splitlines():
    m = re.search(r"remark: .*?:\d+:\d+:\s+(.*?) \[-Rpass", line) or re.search(r"remark:\s+(.*?) \[-Rpass", line)
    if not m:
        m = re.search(r":\d+:\d+:\s+(.*?)\s+\[-Rpass", line)
    if not m:
        continue
    t = m.group(1).strip()
    if t.startswith("Function Name:") or t.startswith("Name:"):
        if cur:
            rows.append(cur)
        cur = {"name": t.split(":", 1)[1].strip()}
    elif ":" in t:
        k, v = t.split(":", 1)
        cur[k.strip()] = v.strip()
if cur:
    rows.append(cur)


def strip_arguments(name):
    """The demangled name without its trailing argument list: `sah::(anonymous namespace)::k<true>(sah::Args)` keeps everything up to
    the parenthesis that matches the last one."""
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i]
    return name


for r in rows:
    name = subprocess.run(["c++filt", r["name"]], stdout=subprocess.PIPE, text=True).stdout.strip()
    name = strip_arguments(name)
    print(f"{name:60s} VGPR {r.get('VGPRs','?'):>4} AGPR {r.get('AGPRs','?'):>3} SGPR {r.get('TotalSGPRs', r.get('SGPRs','?')):>4} "
          f"scratch {r.get('ScratchSize [bytes/lane]','?'):>5} occ {r.get('Occupancy [waves/SIMD]','?'):>2} LDS {r.get('LDS Size [bytes/block]','?'):>6} "
          f"code {code_bytes.get(r['name'], '?'):>6}")
