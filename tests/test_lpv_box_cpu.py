"""The fast Lighting kernel's per-wave LPV texel box (androidrenderer_amd/csrc/lpv_box.hpp) on the host: tests/cpp/lpv_box_check.cpp includes the
very header the kernel includes and checks, for volumes of 32 x 32 x 32, 128 x 32 x 32 and 1 x 1 x 1, every reference base and every pixel base,
that a pixel is served exactly when both taps of every axis are inside the box, that every staged chunk lies inside the padded gather copy, that
every LDS offset lies inside the wave's region and is 16-byte aligned, that the written chunks tile the region and that a tap reads the texel
lpv_fetch_packed would load; and the rule that names the reference lane."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lpv_box_program(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "cpp", "lpv_box_check.cpp"), tmp_path / "lpv_box_check"
    cxx = next(c for c in ("g++", "c++", "/opt/rocm/llvm/bin/clang++") if subprocess.run(["which", c], capture_output=True).returncode == 0 or os.path.exists(c))
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)], timeout=300)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "lpv_box ok" in run.stdout
    for volume in ("32 x 32 x 32", "128 x 32 x 32", "1 x 1 x 1"):
        assert f"volume {volume}:" in run.stdout
