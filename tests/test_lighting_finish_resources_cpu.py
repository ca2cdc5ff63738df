"""What the compiler made of the fast Lighting kernel's bodies (csrc/lighting.hip), read from the code object's metadata and the compiler's
resource remarks through tools/kernel_resources.py — lighting.hip compiled for gfx950 with the library's own options (androidrenderer_amd/build.py).

  - every FINISH body k_lighting_fast<.., true, true> is a kernel without a private segment: .private_segment_fixed_size 0, no VGPR spill, at most
    128 VGPRs and four waves per SIMD (it reads its finish's uniforms late: FinishArgs) — a wave launched with a private segment it never touches,
    and the SGPR spills behind it, were the FINISH bodies' cost over their twins (profiles/finish_twin.txt);
  - every other body of k_lighting_fast, and k_lighting_fixup, is the kernel it was: registers, scratch and occupancy as recorded for the parent
    commit in profiles/strays_inline_kernel_resources.txt (its column "this, in front of a fix-up launch").
Metadata only: nothing here looks at the instruction stream."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "strays_inline_kernel_resources.txt")


@pytest.fixture(scope="module")
def kernels():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernel_resources(os.path.join(ROOT, "androidrenderer_amd", "csrc", "lighting.hip"))
    out = {}
    for r in rows:
        m = re.search(r"(k_lighting_\w+<[^>]*>)$", r["name"])
        if m:
            out[m.group(1)] = r
    return out


def _recorded():
    """body -> (VGPR, SGPR, scratch, waves per SIMD) of the parent commit: the second group of six numbers of each line of the record"""
    out = {}
    for line in open(RECORD):
        m = re.match(r"(k_lighting_(?:fast|fixup)<[^>]*>)\s+(.*)$", line)
        if not m:
            continue
        nums = [int(t) for t in m.group(2).split() if t.isdigit()]
        assert len(nums) >= 12, line
        name = m.group(1)
        if name.startswith("k_lighting_fast"):
            name = name[:-1] + ", false>"  # the record names the body in front of a fix-up launch as the parent of ITS parent did
        out[name] = tuple(nums[6:10])
    return out


def test_the_record_lists_every_body():
    rec = _recorded()
    assert len(rec) == 54 and sum(1 for k in rec if k.startswith("k_lighting_fixup")) == 18


def test_finish_bodies_have_no_private_segment(kernels):
    finish = {k: r for k, r in kernels.items() if re.fullmatch(r"k_lighting_fast<\d, \d, \d, true, true>", k)}
    assert len(finish) == 18, sorted(finish)
    bad = []
    for k, r in sorted(finish.items()):
        print(f"{k}: private segment {r['private_segment']}, VGPRs {r['meta_vgpr']}, VGPR spills {r['vgpr_spills']}, SGPR spills {r['sgpr_spills']}, occupancy {r['occupancy']}")
        assert None not in (r["private_segment"], r["meta_vgpr"], r["vgpr_spills"], r["occupancy"]), f"{k}: metadata not found"
        if not (r["private_segment"] == 0 and r["meta_vgpr"] <= 128 and r["vgpr"] <= 128 and r["occupancy"] == 4 and r["vgpr_spills"] == 0 and r["scratch"] == 0):
            bad.append(k)
    assert not bad, bad


def test_other_bodies_are_the_kernels_they_were(kernels):
    rec = _recorded()
    differ = []
    for name, want in sorted(rec.items()):
        assert name in kernels, f"{name} is in the record and not in the library"
        r = kernels[name]
        got = (r["vgpr"], r["sgpr"], r["scratch"], r["occupancy"])
        if got != want or r["private_segment"] != want[2]:
            differ.append((name, want, got, r["private_segment"]))
    assert not differ, differ
    others = [k for k in kernels if k.startswith(("k_lighting_fast", "k_lighting_fixup")) and not k.endswith("true, true>")]
    assert sorted(others) == sorted(rec)
