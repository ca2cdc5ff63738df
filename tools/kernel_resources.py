"""Print per-kernel register/LDS/occupancy usage for a HIP source (hipcc -Rpass-analysis=kernel-resource-usage), each kernel's code
length in bytes (the size of its symbol in the device object) and what the code object's metadata note says of it (private segment size, spill
counts), compiled with the library's options (androidrenderer_amd/build.py: FLAGS and the per-source SOURCE_FLAGS of the file's name).

    python tools/kernel_resources.py androidrenderer_amd/csrc/lighting.hip

As a module (tests/test_lighting_finish_resources_cpu.py): kernel_resources(src) returns one record per kernel."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import build as hip_build  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


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


def parse_remarks(text):
    """-Rpass-analysis=kernel-resource-usage remarks -> {mangled name: {remark field: value}}"""
    rows, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: .*?:\d+:\d+:\s+(.*?) \[-Rpass", line) or re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            m = re.search(r":\d+:\d+:\s+(.*?)\s+\[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:") or t.startswith("Name:"):
            cur = rows.setdefault(t.split(":", 1)[1].strip(), {})
        elif ":" in t and cur is not None:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


def parse_metadata(notes):
    """`llvm-readelf --notes` of a device object -> {mangled name: {metadata key: value}} for the scalar keys of each entry of amdhsa.kernels
    (.private_segment_fixed_size, .vgpr_count, .sgpr_count, .vgpr_spill_count, .sgpr_spill_count, .group_segment_fixed_size, ...)"""
    kernels, cur, inside = {}, None, False
    for line in notes.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if line and not line.startswith(" "):  # the next top-level key
            inside = False
            continue
        m = re.match(r"^  ([- ]) (\.\w+):\s*(.*)$", line)  # (deeper lines are the entries of .args)
        if not m:
            continue
        if m.group(1) == "-":
            cur = {}
        cur[m.group(2)] = m.group(3).strip().strip("'\"")
        if m.group(2) == ".name":
            kernels[cur[".name"]] = cur
    return kernels


def kernel_resources(src, extra_flags=()):
    """Compiles the device half of `src` alone with the library's options and returns a list of records, one per kernel:
    name (demangled, without arguments), mangled, vgpr, agpr, sgpr, scratch (bytes per lane), occupancy (waves per SIMD), lds (bytes per
    workgroup) — the compiler's resource remarks —, code_bytes (the symbol's size), and from the code object's metadata note private_segment
    (.private_segment_fixed_size), vgpr_spills, sgpr_spills, meta_vgpr (.vgpr_count)."""
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "device.o")
        cmd = ([HIPCC] + hip_build.FLAGS + hip_build.SOURCE_FLAGS.get(os.path.basename(src), []) + list(extra_flags) +
               ["--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj, "-Rpass-analysis=kernel-resource-usage"])
        run = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        if run.returncode != 0 or not os.path.exists(obj):
            raise RuntimeError(f"{' '.join(cmd)} failed:\n{run.stderr[-4000:]}")
        code_bytes = {}
        syms = subprocess.run([READELF, "-s", "--wide", obj], stdout=subprocess.PIPE, text=True, check=True).stdout
        for line in syms.splitlines():
            f = line.split()
            if len(f) == 8 and f[3] == "FUNC":
                code_bytes[f[7]] = int(f[2], 0)
        meta = parse_metadata(subprocess.run([READELF, "--notes", obj], stdout=subprocess.PIPE, text=True, check=True).stdout)
    remarks = parse_remarks(run.stderr)
    names = list(remarks)
    demangled = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.splitlines() if names else []

    def num(v):
        return int(v) if v is not None and re.fullmatch(r"-?\d+", v) else None

    out = []
    for mangled, pretty in zip(names, demangled):
        r, m = remarks[mangled], meta.get(mangled, {})
        out.append({"name": strip_arguments(pretty.strip()), "mangled": mangled, "vgpr": num(r.get("VGPRs")), "agpr": num(r.get("AGPRs")),
                    "sgpr": num(r.get("TotalSGPRs", r.get("SGPRs"))), "scratch": num(r.get("ScratchSize [bytes/lane]")),
                    "occupancy": num(r.get("Occupancy [waves/SIMD]")), "lds": num(r.get("LDS Size [bytes/block]")), "code_bytes": code_bytes.get(mangled),
                    "private_segment": num(m.get(".private_segment_fixed_size")), "vgpr_spills": num(m.get(".vgpr_spill_count")),
                    "sgpr_spills": num(m.get(".sgpr_spill_count")), "meta_vgpr": num(m.get(".vgpr_count"))})
    return out


def main():
    def s(v):
        return "?" if v is None else v

    for r in kernel_resources(sys.argv[1]):
        print(f"{r['name']:60s} VGPR {s(r['vgpr']):>4} AGPR {s(r['agpr']):>3} SGPR {s(r['sgpr']):>4} scratch {s(r['scratch']):>5} occ {s(r['occupancy']):>2} "
              f"LDS {s(r['lds']):>6} code {s(r['code_bytes']):>6} private {s(r['private_segment']):>4} spills v {s(r['vgpr_spills']):>3} s {s(r['sgpr_spills']):>3}")


if __name__ == "__main__":
    main()
