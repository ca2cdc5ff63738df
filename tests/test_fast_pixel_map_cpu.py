"""The fast Lighting kernel's thread -> pixel map (androidrenderer_amd/csrc/fast_pixel_map.hpp) on the host: tests/cpp/fast_pixel_map_check.cpp
includes the very header the kernels and api.cpp include and checks, shape by shape, that the map is a bijection onto the thread groups, that
every aligned run of 64 thread indices inside the tiled region is one tile — 64 pixels x ppt rows, the shape the header keeps — with lanes
row-major, that the rows behind the last full band and every launch with tile_rows 0 keep the linear split, and that the multiply-high agrees
with the plain divide on either side of its limit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fast_pixel_map_program(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "cpp", "fast_pixel_map_check.cpp"), tmp_path / "fast_pixel_map_check"
    cxx = next(c for c in ("g++", "c++", "/opt/rocm/llvm/bin/clang++") if subprocess.run(["which", c], capture_output=True).returncode == 0 or os.path.exists(c))
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)], timeout=300)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "fast_pixel_map ok" in run.stdout
    # the shapes the program is there for did take the branches they were chosen for
    assert "3840 x 2160 at 4 px/thread: tile_rows 4, row_magic yes" in run.stdout
    assert "3840 x 291 at 1 px/thread: tile_rows 1, row_magic yes" in run.stdout
    assert "3840 x 292 at 1 px/thread: tile_rows 1, row_magic no" in run.stdout
    assert "3840 x 4663 at 4 px/thread: tile_rows 4, row_magic no" in run.stdout
    assert "128 x 23 at 4 px/thread: tile_rows 4" in run.stdout
    assert "72 x 16 at 4 px/thread: tile_rows 0" in run.stdout
