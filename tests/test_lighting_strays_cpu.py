"""CPU-only: the debug knob that says how the fast Lighting kernel's strays are finished (sah_debug_set's `strays`, lib.Context.debug_set)
takes its three values and refuses every other, and the ABI structs keep their sizes beside it."""
import ctypes as C

import pytest

from androidrenderer_amd import _abi, lib


def _context():
    """a Context without a device where there is none, on cuda:0 where there is one: the knob is host state either way"""
    L = lib.load()
    h = lib.create_detached()
    if h is None:  # a HIP device is present
        return lib.Context(device=0)
    ctx = lib.Context.__new__(lib.Context)
    ctx.lib, ctx.handle = L, h
    return ctx


def test_strays_knob_takes_its_three_values_and_refuses_others():
    ctx = _context()
    L = ctx.lib
    try:
        assert (_abi.DEBUG_STRAYS_AUTO, _abi.DEBUG_STRAYS_LAUNCH, _abi.DEBUG_STRAYS_INLINE) == (0, 1, 2)
        assert list(lib.Context.STRAYS_MODES) == ["auto", "launch", "inline"]
        for mode in (0, 1, 2):
            assert L.sah_debug_set(ctx.handle, 0, 0, mode) == _abi.SAH_OK
        for bad in (-1, 3, 4, 255, 2 ** 31 - 1, -2 ** 31):
            assert L.sah_debug_set(ctx.handle, 0, 0, bad) == _abi.SAH_ERR_INVALID_ARGUMENT, bad
            assert b"strays" in L.sah_last_error(ctx.handle)
        assert L.sah_debug_set(None, 0, 0, 0) == _abi.SAH_ERR_INVALID_ARGUMENT
        for name in ("auto", "launch", "inline"):
            ctx.debug_set(strays=name)
        ctx.debug_set(force_general=True, force_ppt=4)  # (the two older knobs alone, as every earlier caller writes it)
        for bad in ("", "Inline", "fixup", None, 1, True):
            with pytest.raises(ValueError):
                ctx.debug_set(strays=bad)
        ctx.debug_set()
    finally:
        ctx.close()


def test_dispatch_report_names_the_strays_word_last():
    assert lib.Context.DISPATCH_FIELDS[-1] == "strays" and len(lib.Context.DISPATCH_FIELDS) == 13
    assert len(set(lib.Context.DISPATCH_FIELDS)) == 13


def test_struct_sizes_still_match():
    # (tests/test_abi.py's list: the knob and the report word are debug hooks, sah_lighting's ABI and LightingDesc stay as they are)
    assert C.sizeof(_abi.ViewData) == 432
    assert C.sizeof(_abi.SunLightConstants) == 640
    assert C.sizeof(_abi.LpvCascadeMatrices) == 256
    assert C.sizeof(_abi.ProbeCascade) == 16
    assert C.sizeof(_abi.PointLight) == 32
    assert C.sizeof(_abi.Plane) == 24
    assert C.sizeof(_abi.Volume) == 32
    assert lib.load().sah_abi_version() == 6
    names = [n for n, _ in _abi.LightingDesc._fields_]
    assert "gbuffer" in names and not any("stray" in n for n in names)  # (the descriptor has no field for the knob)
