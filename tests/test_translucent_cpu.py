"""Alpha-blended geometry (include/sah_translucent.h) without a GPU: the export, the header and the descriptor, the mesh helpers, an argument
fuzz in a child process, and the reference composition (tests/translucent_ref.py) on the CPU oracle — the properties of the contract it must
show by itself, and its committed fixture."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib, mesh, scene
from tests import translucent_ref as ref
from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_translucent as gen  # noqa: E402

HEADER = os.path.join(ROOT, "include", "sah_translucent.h")
W, H = 96, 54
BACKEND = ref.OracleBackend()


# ---- exports, header, structure -----------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.TRANSLUCENT_EXPORTS)
    header = open(HEADER).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.TRANSLUCENT_EXPORTS) == ["sah_translucent_render"]
    assert not set(lib.TRANSLUCENT_EXPORTS) & set(lib.EXPORTS)
    hip_h = open(os.path.join(ROOT, "include", "sah_hip.h")).read()
    assert "sah_translucent" not in hip_h and "TRANSLUCENT" not in hip_h and re.search(r"#define\s+SAH_ABI_VERSION\s+6\b", hip_h)  # sah_hip.h stays as it is
    assert re.search(r"#define\s+SAH_PRIMITIVE_TYPE_TRANSLUCENT\s+2\b", header) and _abi.PRIMITIVE_TYPE_TRANSLUCENT == 2
    assert "ABI-defined" in header and "Off by default" in header and "Not built" in header
    assert "split_translucent" in header  # the header says who hands the other entry points the scene without its type-2 primitives


@pytest.mark.parametrize("language", ["c", "c++"])
def test_header_compiles_and_the_descriptor_is_three_pointers(tmp_path, language):
    src = tmp_path / ("use.c" if language == "c" else "use.cpp")
    check = "_Static_assert" if language == "c" else "static_assert"
    offsets = [("lighting", 0), ("scene", 8), ("stats", 16)]
    src.write_text('#include <stddef.h>\n#include "sah_translucent.h"\n'
                   f'{check}(sizeof(sah_translucent_desc) == 24, "sah_translucent_desc");\n' +
                   "".join(f'{check}(offsetof(sah_translucent_desc, {n}) == {o}, "{n}");\n' for n, o in offsets) +
                   "int use(sah_ctx* c, const sah_translucent_desc* d) { return sah_translucent_render(c, d) + SAH_PRIMITIVE_TYPE_TRANSLUCENT; }\n")
    clang = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else "cc"
    subprocess.check_call([clang, "-x", language, "-std=c11" if language == "c" else "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)], timeout=120)
    assert C.sizeof(_abi.TranslucentDesc) == 24
    assert [(n, getattr(_abi.TranslucentDesc, n).offset) for n, _ in _abi.TranslucentDesc._fields_] == offsets


def test_refusals_on_a_context_without_a_device():
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        pytest.skip("a HIP device is present")
    INV = _abi.SAH_ERR_INVALID_ARGUMENT
    d, g = _abi.LightingDesc(), _abi.SceneGeometry()
    assert L.sah_translucent_render(None, None) == INV and L.sah_translucent_render(h, None) == INV
    for t in (_abi.TranslucentDesc(None, C.pointer(g), None), _abi.TranslucentDesc(C.pointer(d), None, None), _abi.TranslucentDesc(C.pointer(d), C.pointer(g), None)):
        assert L.sah_translucent_render(h, C.byref(t)) == INV  # (the last: an empty lighting descriptor, sah_lighting's refusal)
    L.sah_destroy(h)


@pytest.mark.parametrize("seed", [59])
def test_no_argument_combination_crashes_the_entry(seed):
    stdout = support.run_fuzz_child("translucent_fuzz_child.py", seed, 2000)
    assert not re.search(r"\bok: \d", stdout)  # (a detached context never launches)
    assert "unsupported" in stdout and "invalid_argument" in stdout  # the entry's own checks were reached


# ---- the mesh helpers -----------------------------------------------------------------------------------------------------------------------
def test_split_translucent_keeps_order_and_shares_the_streams():
    arrays = ref.scene_panes().arrays()
    opaque, translucent = mesh.split_translucent(arrays)
    types = arrays["primitives"]["type"]
    assert (opaque["primitives"]["type"] != ref.T).all() and (translucent["primitives"]["type"] == ref.T).all()
    assert len(translucent["primitives"]) == int((types == ref.T).sum()) == 7 and len(opaque["primitives"]) + 7 == len(types)
    assert opaque["primitives"].tobytes() == arrays["primitives"][types != ref.T].tobytes()
    assert translucent["primitives"].tobytes() == arrays["primitives"][types == ref.T].tobytes()
    for k in ("positions", "vertex_data", "indices", "materials"):
        assert opaque[k] is arrays[k] and translucent[k] is arrays[k]
    plain = mesh.atrium(2).arrays()
    o, t = mesh.split_translucent(plain)
    assert o["primitives"].tobytes() == plain["primitives"].tobytes() and len(t["primitives"]) == 0


def test_add_primitive_takes_the_type_and_the_atrium_is_unchanged_by_default():
    m = mesh.Mesh()
    i = ref.pane(m, 0.0, (0, 1), (0, 1), m.add_material(mesh.material()))
    assert m.primitives[i]["type"] == _abi.PRIMITIVE_TYPE_TRANSLUCENT == 2
    a, b = mesh.atrium(1).arrays(), mesh.atrium(1, translucent_fraction=0.0).arrays()
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("positions", "vertex_data", "indices", "primitives", "materials"))
    g = mesh.atrium(1, translucent_fraction=0.1).arrays()
    n = int((g["primitives"]["type"] == ref.T).sum())
    assert n == int(len(a["primitives"]) * 0.1) == 3 and len(g["primitives"]) == len(a["primitives"]) and len(g["materials"]) == 7
    assert g["positions"].tobytes() == a["positions"].tobytes()


def test_sort_back_to_front_is_by_view_depth_farthest_first_and_stable():
    view = scene.SceneView.default(W, H)  # at (-7, 1, 0) looking along +x
    m = mesh.Mesh()
    mat = m.add_material(mesh.material())
    xs = [-2.0, 5.0, 1.0, 5.0, -4.0, 1.0]
    for k, x in enumerate(xs):
        ref.pane(m, x, (0, 1), (k, k + 1), mat)
    # an instance whose model matrix moves it farthest of all
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 20.0
    m.add_instance(0, far.T.reshape(16))
    arrays = m.arrays()
    out = mesh.sort_back_to_front(arrays, view.gpu_data.view[:])
    order = [int(p["first_index"]) // 6 for p in out["primitives"]]
    assert order == [0, 1, 3, 2, 5, 0, 4]  # the instance of 0 (x = 18), the two at 5 in list order, the two at 1 in list order, -2, -4
    assert out["primitives"][0]["model"][12] == 20.0 and out["positions"] is arrays["positions"]
    assert arrays["primitives"].tobytes() == m.arrays()["primitives"].tobytes()  # the input is left alone


# ---- the composition's own properties -------------------------------------------------------------------------------------------------------
def _frame(m, **kw):
    return ref.Frame(BACKEND, m, W, H, **kw)


def test_alpha_code_0_leaves_lit_alone_and_255_over_a_finite_background_gives_the_fragment_colour():
    fr = _frame(ref.scene_alpha_codes())
    lit, blended = fr.compose()
    ref.assert_preconditions(fr, lit, blended, min_changed=0.2, min_depth=1)
    records = ref.single_triangle_records(fr.translucent)
    materials = fr.translucent["materials"].copy()
    materials["opacity_threshold"] = -1.0
    seen = set()
    for i in range(len(records)):
        gb = BACKEND.gbuffer(dict(fr.translucent, primitives=records[i:i + 1], materials=materials), fr.f.view, W, H)
        on = gb["depth"] > fr.depth
        assert on.any()
        code = np.unique(gb["color"][..., 3][on])
        assert len(code) == 1
        seen.add(int(code[0]))
        if code[0] == 0:
            assert lit[on].tobytes() == fr.lit0[on].tobytes() and (blended[on] == 0).all()
        if code[0] == 255:
            src = BACKEND.lighting(fr.f, gb)
            assert not ((fr.lit0[on] & 0x7fff) >= 0x7c00).any()
            assert np.array_equal(lit[on].view(np.float16), src[on].view(np.float16))  # (S * 1) + (D * 0), D finite: the value of S
            assert (lit[on] != fr.lit0[on]).any()
    assert seen == {0, 1, 128, 255}


def test_a_fragment_at_exactly_the_opaque_depth_is_dropped():
    m = mesh.Mesh()
    wall = m.add_material(mesh.material(base=(0.7, 0.6, 0.5, 1.0)))
    ref.pane(m, -2.0, (-2.0, 4.0), (-4.0, 3.0), wall, ptype=_abi.PRIMITIVE_TYPE_SOLID)
    ref.pane(m, -2.0, (-2.0, 4.0), (-4.0, 3.0), ref.glass(m, (0.1, 0.9, 0.2, 0.8)))   # the same vertices: the same depth at every pixel
    ref.pane(m, -2.0, (-2.0, 4.0), (3.0, 5.0), ref.glass(m, (0.1, 0.9, 0.2, 0.8)))    # beside the wall, over the sky: blended
    fr = _frame(m)
    lit, blended = fr.compose()
    on_wall = fr.depth > 0
    assert on_wall.mean() > 0.2 and lit[on_wall].tobytes() == fr.lit0[on_wall].tobytes() and (blended[on_wall] == 0).all()
    assert (blended[~on_wall] == 1).any()


def test_two_overlapping_layers_swapped_give_another_image():
    a, b = _frame(ref.scene_stack(2)), _frame(ref.scene_stack(2, reverse=True))
    la, na = a.compose()
    lb, nb = b.compose()
    assert a.lit0.tobytes() == b.lit0.tobytes() and np.array_equal(na, nb) and na.max() == 2
    both = na == 2
    assert (la[both] != lb[both]).any() and la[na == 1].tobytes() == lb[nb == 1].tobytes()


def test_rows_limit_the_pixels_written():
    fr = _frame(ref.scene_stack(3))
    full, _ = fr.compose()
    for rows in ((10, 30), (0, 1), (53, 54), (20, 20)):
        part, _ = fr.compose(rows=rows)
        want = np.array(fr.lit0)
        want[rows[0]:rows[1]] = full[rows[0]:rows[1]]
        assert part.tobytes() == want.tobytes(), rows


def test_the_stack_is_at_least_five_fragments_deep():
    fr = _frame(ref.scene_stack(6))
    lit, blended = fr.compose()
    ref.assert_preconditions(fr, lit, blended, min_changed=0.2, min_depth=5)


def test_the_near_plane_scene_is_clipped_and_blended():
    fr = _frame(ref.scene_near())
    lit, blended = fr.compose()
    ref.assert_preconditions(fr, lit, blended, min_changed=0.2, min_depth=3)
    assert (blended[0] > 0).all()  # the sheet fills the row under the camera (the projection has no y flip: world down is row 0): it runs on through the near plane


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_composition_gives():
    fx = np.load(gen.FIXTURE)
    assert os.path.getsize(gen.FIXTURE) < 500_000
    data = gen.generate()
    assert sorted(fx.files) == sorted(data)
    for k in data:
        assert fx[k].dtype == data[k].dtype and fx[k].tobytes() == data[k].tobytes(), k
