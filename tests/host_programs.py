"""The C++ programs of tests/cpp that run frames through the host façade (include/sah_host.hpp): the one place that knows how such a
program is compiled and when a built one is stale.  __graft_entry__.build() builds NAMES in place; a test asks for its program with
host_program(name, tmp_path) and gets the built one, or one compiled into its tmp_path where that is missing or older than its sources."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = ("/opt/rocm/bin/hipcc",)

# built by build(), so that they travel with the tree to where the GPU tests run
NAMES = ("host_frame", "host_raster", "host_vrsaa", "host_hi_z", "host_rt_refit", "host_gbuffer_motion", "host_taa", "host_taa_upscale", "host_ssao",
         "host_rt_denoise", "host_exposure", "host_rtgi_denoise", "host_sharpen", "host_lighting_vrs", "host_ssr", "host_motion_blur", "host_sun_shafts",
         "host_translucent")


def host_program(name, tmp_path=None, root=ROOT, compiler=HIPCC):
    """The path of the executable of tests/cpp/<name>.cpp: the one beside the source if it is no older than the source and every header of
    include/, otherwise one compiled now — into tmp_path, or in place where tmp_path is None."""
    built = os.path.join(root, "tests", "cpp", name)
    src, include, libdir = built + ".cpp", os.path.join(root, "include"), os.path.join(root, "androidrenderer_amd")
    deps = [src] + glob.glob(os.path.join(include, "*.h")) + glob.glob(os.path.join(include, "*.hpp"))
    if os.path.exists(built) and os.path.getmtime(built) >= max(os.path.getmtime(d) for d in deps):
        return built
    exe = built if tmp_path is None else os.path.join(str(tmp_path), name)
    subprocess.check_call([*compiler, "-std=c++17", "-O2", "-I", include, src, "-o", exe, "-L", libdir, "-lsah_hip", f"-Wl,-rpath,{libdir}"], timeout=600)
    return exe
