"""The helpers the tests share (tests/support.py, tests/host_programs.py, the fuzz children's loop in tests/abi_fuzz_child.py), without a
GPU: the byte comparison and its message on the values where == on floats misleads, the malformed copies of a plane, the loop of the fuzz
children on a table of its own, and the staleness rule of the C++ programs on a stub tree with a stub compiler."""
import os
import sys
import types

import numpy as np

from androidrenderer_amd import _abi
from tests import host_programs, support
from tests.abi_fuzz_child import run_calls

f32 = np.float32


# ---- same / differs -------------------------------------------------------------------------------------------------------------------------
def test_same_tells_the_zeros_apart_and_a_nan_equals_itself():
    pos, neg = np.zeros((3, 4), f32), np.zeros((3, 4), f32)
    neg[1, 2] = -0.0
    assert (pos == neg).all() and not support.same(pos, neg)
    nan = np.full((3, 4), np.uint32(0x7FC00123)).view(f32)
    assert not (nan == nan.copy()).any() and support.same(nan, nan.copy())
    assert support.same(nan.tobytes(), nan) and support.same(nan, nan.tobytes()) and not support.same(nan.tobytes(), pos)
    assert support.same(nan[:, ::2], np.ascontiguousarray(nan[:, ::2]))  # the bytes of the texels, not of the memory they lie in


def test_differs_counts_texels_by_their_bytes_float32():
    a = np.full((5, 7), np.uint32(0x7FC00000)).view(f32)
    b = a.copy()
    b.view(np.uint32)[3, 2] ^= 1  # one payload bit of a NaN: != says every texel differs, the bytes say one
    assert (a != b).all() and not support.same(a, b)
    assert support.differs(a, b) == "1 of 35 texels differ, first (y, x) at [[3, 2]]"
    b[0, 6] = -0.0
    a[0, 6] = 0.0
    assert support.differs(a, b) == "2 of 35 texels differ, first (y, x) at [[0, 6], [3, 2]]"


def test_differs_counts_texels_by_their_bytes_uint16_channels():
    a = np.arange(4 * 6 * 4, dtype=np.uint16).reshape(4, 6, 4)
    b = a.copy()
    b[2, 5, 3] += 1
    b[2, 5, 0] += 1  # two channels of one texel
    b[3, 0, 1] ^= 0x8000
    assert support.differs(a, b) == "2 of 24 texels differ, first (y, x) at [[2, 5], [3, 0]]"
    assert support.differs(a[1:], b[1:]) == "2 of 18 texels differ, first (y, x) at [[1, 5], [2, 0]]"  # a band of rows
    assert support.differs(a, a.copy()).startswith("0 of 24 ")


# ---- retyped / resized ------------------------------------------------------------------------------------------------------------------------
def _fields(s):
    return {n: getattr(s, n) for n, _ in s._fields_}


def test_retyped_and_resized_change_their_fields_only():
    p = _abi.Plane(0x7F0000001000, 97, 61, 400, _abi.FORMAT_R16G16_SFLOAT)
    before = _fields(p)
    r = support.retyped(p, _abi.FORMAT_R32_SFLOAT)
    assert type(r) is _abi.Plane and _fields(r) == dict(before, format=_abi.FORMAT_R32_SFLOAT)
    z = support.resized(p, 13, 8)
    assert type(z) is _abi.Plane and _fields(z) == dict(before, width=13, height=8)
    assert _fields(p) == before  # copies: the plane they were made from stands
    v = _abi.Volume(0x7F0000002000, 128, 32, 4, 1024, 32768, _abi.FORMAT_D16_UNORM)
    rv = support.retyped(v, _abi.FORMAT_R16G16B16A16_SFLOAT)
    assert type(rv) is _abi.Volume and _fields(rv) == dict(_fields(v), format=_abi.FORMAT_R16G16B16A16_SFLOAT)


# ---- the fuzz children's loop ---------------------------------------------------------------------------------------------------------------------
def test_run_calls_counts_statuses_and_clears_keep_every_iteration(capsys):
    fuzz = types.SimpleNamespace(keep=[])
    kept, order = [], []

    def entry(name, rc):
        def call():
            kept.append(len(fuzz.keep))
            order.append(name)
            fuzz.keep.append(object())
            return rc
        return call
    calls = {"sah_b": entry("sah_b", _abi.SAH_ERR_INVALID_ARGUMENT), "sah_a": entry("sah_a", _abi.SAH_ERR_HIP)}
    assert run_calls(calls, 7, 3, fuzz) == 0
    assert order == ["sah_a", "sah_b"] * 3          # sorted, per iteration
    assert kept == [0, 1] * 3 and fuzz.keep == []   # what an iteration kept is gone before the next
    out = capsys.readouterr().out.splitlines()
    assert out == [f"{'sah_a':26s} hip: 3", f"{'sah_b':26s} invalid_argument: 3", "OK: 3 iterations x 2 entry points, seed 7"]
    assert run_calls({"sah_a": lambda: 0}, 1, 2, fuzz, width=34) == 0
    assert capsys.readouterr().out.splitlines()[0] == f"{'sah_a':34s} ok: 2"


def test_run_calls_fails_on_a_return_that_is_no_status(capsys):
    fuzz = types.SimpleNamespace(keep=[])
    returns = iter([0, -1, 0, 17])
    calls = {"sah_good": lambda: 0, "sah_odd": lambda: next(returns)}
    assert run_calls(calls, 99, 10, fuzz) == 1
    out = capsys.readouterr().out.splitlines()
    assert out == ["FAIL: sah_odd returned 17, not a sah_status (iteration 3, seed 99)"]  # and no OK: line
    assert run_calls({"sah_none": lambda: None}, 5, 1, fuzz) == 1
    assert "FAIL: sah_none returned None, not a sah_status (iteration 0, seed 5)" in capsys.readouterr().out


# ---- host programs ------------------------------------------------------------------------------------------------------------------------------
def _stub_tree(tmp_path):
    """a tree with tests/cpp/host_x.cpp, two headers and a compiler that writes its command line to the path after -o"""
    root = tmp_path / "tree"
    for d in ("tests/cpp", "include", "androidrenderer_amd"):
        (root / d).mkdir(parents=True)
    for f in ("tests/cpp/host_x.cpp", "include/sah_hip.h", "include/sah_host.hpp"):
        (root / f).write_text("")
        os.utime(root / f, (1000, 1000))
    stub = tmp_path / "stub_compiler.py"
    stub.write_text("import sys\nopen(sys.argv[sys.argv.index('-o') + 1], 'w').write(' '.join(sys.argv[1:]))\n")
    return root, (sys.executable, str(stub))


def test_host_program_returns_the_built_one_while_it_is_no_older_than_its_sources(tmp_path):
    root, compiler = _stub_tree(tmp_path)
    built = root / "tests/cpp/host_x"
    built.write_text("built")
    os.utime(built, (1000, 1000))  # as old as its newest source: still good
    out = tmp_path / "out"
    out.mkdir()
    assert host_programs.host_program("host_x", out, root=str(root), compiler=compiler) == str(built)
    assert built.read_text() == "built" and not list(out.iterdir())  # nothing compiled
    for newer in ("tests/cpp/host_x.cpp", "include/sah_hip.h", "include/sah_host.hpp"):  # the source or any header of include/, .h or .hpp
        os.utime(root / newer, (2000, 2000))
        exe = host_programs.host_program("host_x", out, root=str(root), compiler=compiler)
        assert exe == str(out / "host_x") and built.read_text() == "built"
        line = (out / "host_x").read_text()
        assert line.startswith(f"-std=c++17 -O2 -I {root / 'include'} {root / 'tests/cpp/host_x.cpp'} -o {exe} ") and line.endswith(
            f"-L {root / 'androidrenderer_amd'} -lsah_hip -Wl,-rpath,{root / 'androidrenderer_amd'}")
        (out / "host_x").unlink()
        os.utime(root / newer, (1000, 1000))
    assert host_programs.host_program("host_x", out, root=str(root), compiler=compiler) == str(built)


def test_host_program_compiles_a_missing_one_into_tmp_path_or_in_place(tmp_path):
    root, compiler = _stub_tree(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    assert host_programs.host_program("host_x", out, root=str(root), compiler=compiler) == str(out / "host_x")
    assert not (root / "tests/cpp/host_x").exists()
    assert host_programs.host_program("host_x", root=str(root), compiler=compiler) == str(root / "tests/cpp/host_x")  # what build() asks for
    first = os.path.getmtime(root / "tests/cpp/host_x")
    assert first >= 1000 and host_programs.host_program("host_x", root=str(root), compiler=compiler) == str(root / "tests/cpp/host_x")
    assert os.path.getmtime(root / "tests/cpp/host_x") == first  # a second build compiles nothing


def test_names_are_the_programs_with_a_source():
    assert len(host_programs.NAMES) == len(set(host_programs.NAMES)) == 18
    assert all(os.path.exists(os.path.join(host_programs.ROOT, "tests", "cpp", n + ".cpp")) for n in host_programs.NAMES)
