"""The screen-space passes' shared argument rules (androidrenderer_amd/csrc/plane_check.hpp) on the host: tests/cpp/plane_check.cpp includes the
very header the entry points include, nothing of HIP, and checks plane_status for every format, the byte ranges and their overlap (touching,
one shared byte, the gap behind a pitched plane's last row, an end that wraps past 2^64), texel_count_too_large and resolve_rows at their
boundaries.  Built as a plain executable with the address and undefined-behaviour sanitizers; no address it makes up is dereferenced."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_check_program(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "cpp", "plane_check.cpp"), tmp_path / "plane_check"
    cxx = next(c for c in ("g++", "c++", "/opt/rocm/llvm/bin/clang++") if subprocess.run(["which", c], capture_output=True).returncode == 0 or os.path.exists(c))
    # the sanitizers' runtimes linked into the program (clang's default, an option for gcc): a shared runtime refuses to start behind whatever
    # library the environment preloads
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_runtime = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static_runtime
                          + [src, "-o", str(exe)], timeout=300)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "plane_check ok" in run.stdout
