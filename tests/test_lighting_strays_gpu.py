"""The fast Lighting kernel's strays — the pixels it lists for the general restatement — finished by the fix-up launch or by the fast kernel
itself (FastArgs::strays_inline; the launcher's rule: csrc/ctx_cache.hpp, SahStraysRecord): the same bytes either way, each compared with
np.array_equal against the image of the same frame under debug_set(force_general=True); which way a call took is read from the dispatch
report.  Frames as tests/test_lighting_gpu.py::test_fixup_hint_across_calls uses them: a CSM sun and an LPV; "random" lists pixels (roughness
0 under the LPV), "atrium" lists none."""
import numpy as np
import pytest

from androidrenderer_amd import _abi, lib
from tests import lighting_cases as lc, util

pytestmark = pytest.mark.gpu

MODE = dict(sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV)
# (+0 in inverse_projection[12], [13]: the dispatch report then needs nothing from the device, so it can be read inside a stream capture)
CAMERA = dict(edit="plus_zero")
# extent, row range ((0, 0): all).  256 x 8: two workgroups at 4 pixels per thread, a whole band of tiles and nothing else, the smallest launch in
# which a wave's segment index is not 0.  64 x 4 and 64 x 8 with the rows cut: fewer rows than a tile has, and a band of tiles followed by the
# remainder rows of fast_pixel_of.
EXTENTS = {"256x144": (256, 144, (0, 0)), "256x8": (256, 8, (0, 0)), "64x4_rows_1_4": (64, 4, (1, 4)), "64x8_rows_1_8": (64, 8, (1, 8))}
_frames = {}


def _frame(extent, sky, flavour="random", seed=31):
    """the frame, its device arrays and the general kernel's image of it — made once, never changed"""
    key = (extent, sky, flavour, seed)
    if key not in _frames:
        w, h, rows = EXTENTS[extent]
        f = lc.MatrixFrame(w, h, camera=CAMERA, seed=seed, flavour=flavour, sky=sky, **MODE)
        f.row_begin, f.row_end = rows
        if flavour == "random":  # strays in every wave's reach, whatever the random roughness bytes are
            f.arrays["data"].reshape(-1, 4)[::37, 1] = 0
        _frames[key] = [f, f.device_arrays(), None]
    return _frames[key]


def _want(ctx, entry):
    if entry[2] is None:
        ctx.debug_set(force_general=True)
        entry[2] = entry[0].run_hip(ctx, entry[1])
        assert ctx.lighting_dispatch()["family"] == "general"
    return entry[2]


def _run(ctx, f, dev, ppt, strays):
    ctx.debug_set(force_ppt=ppt, strays=strays)
    got = f.run_hip(ctx, dev)
    rep = ctx.lighting_dispatch()
    assert rep["family"] == "fast" and rep["ppt"] == ppt, rep
    return got, rep, ctx.deferred_pixels()


@pytest.fixture
def ctx():
    """a context of the test's own on torch's current stream: its record of recent calls starts empty"""
    import torch
    c = lib.Context(device=0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    torch.cuda.synchronize()
    c.close()


@pytest.mark.parametrize("sky", [True, False], ids=["sky", "no_sky"])
@pytest.mark.parametrize("extent", list(EXTENTS))
@pytest.mark.parametrize("ppt", [4, 2, 1])
def test_inline_finish_is_exact(hip_ctx, ppt, extent, sky):
    entry = _frame(extent, sky)
    f, dev = entry[0], entry[1]
    want = _want(hip_ctx, entry)
    try:
        by_launch, rep_l, n_launch = _run(hip_ctx, f, dev, ppt, "launch")
        inline, rep_i, n_inline = _run(hip_ctx, f, dev, ppt, "inline")
    finally:
        hip_ctx.debug_set()
    print(f"ppt {ppt} {extent} sky {sky}: {n_inline} listed; launch {rep_l['strays']}, inline {rep_i['strays']}")
    assert rep_l["strays"] == "launch"
    # (a body without a sky bound keeps the fix-up launch whatever is asked: csrc/lighting.hip, strays_inline_body)
    assert rep_i["strays"] == ("inline" if sky else "launch")
    assert n_inline > 0 and n_inline == n_launch
    assert np.array_equal(by_launch, want)
    assert np.array_equal(inline, want), f"{int((inline != want).any(-1).sum())} pixels differ from the general kernel's"


@pytest.mark.parametrize("ppt", [4, 2, 1])
def test_inline_finish_on_a_pitched_offset_lit_target(hip_ctx, ppt):
    entry = _frame("256x144", True)
    f, dev = entry[0], entry[1]
    want = _want(hip_ctx, entry)
    try:
        f.pitch = {"lit": dict(row_pad=48, offset=32)}  # (multiples of 16: every pixel-per-thread setting stays available)
        got, rep, n = _run(hip_ctx, f, dev, ppt, "inline")  # (run_hip asserts the padding)
    finally:
        f.pitch = {}
        hip_ctx.debug_set()
    assert rep["strays"] == "inline" and n > 0
    assert np.array_equal(got, want)


def _tile_frame(listed):
    """`listed` None: the random frame with every roughness byte of one 64 x 4 tile 0 — at 4 pixels per thread one wave lists its 256 pixels,
    four dealing passes; a number: the atrium frame (which lists nothing) with that many roughness bytes of one all-surface tile 0"""
    key = ("tile", listed)
    if key not in _frames:
        f = lc.MatrixFrame(256, 144, camera=CAMERA, seed=32 if listed else 31, flavour="atrium" if listed else "random", sky=True, **MODE)
        depth, rough = f.arrays["depth"], f.arrays["data"][..., 1]
        if listed is None:
            rough[8:12, 128:192] = 0
        else:
            assert (rough[depth != 0] != 0).all()  # (no surface pixel of the atrium is listed; its sky pixels are the sky workgroups')
            y0, x0 = next((y, x) for y in range(0, 144, 4) for x in range(0, 256, 64) if (depth[y:y + 4, x:x + 64] != 0).all())
            tile = rough[y0:y0 + 4, x0:x0 + 64]
            flat = np.zeros(256, bool)
            flat[(np.arange(listed) * 7) % 256] = True  # 7 is coprime to 256: `listed` distinct pixels, spread over the tile's lanes and slots
            tile[flat.reshape(4, 64)] = 0
            assert int((rough[depth != 0] == 0).sum()) == listed
        _frames[key] = [f, f.device_arrays(), None]
    return _frames[key]


@pytest.mark.parametrize("listed", [None, 64, 65], ids=["whole_tile", "64", "65"])
def test_inline_finish_deals_more_than_one_pass(hip_ctx, listed):
    entry = _tile_frame(listed)
    f, dev = entry[0], entry[1]
    want = _want(hip_ctx, entry)
    try:
        got, rep, n = _run(hip_ctx, f, dev, 4, "inline")
    finally:
        hip_ctx.debug_set()
    assert rep["strays"] == "inline"
    if listed is None:
        assert n >= 256
    else:
        assert n == listed
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} pixels differ from the general kernel's"


def test_auto_follows_the_record_of_recent_calls(ctx):
    ea, eb = _frame("256x144", True, "random", 31), _frame("256x144", True, "atrium", 32)
    want_a, want_b = _want(ctx, ea), _want(ctx, eb)
    ctx.debug_set()  # strays="auto"
    forms = []

    def call(entry, want, rows=(0, 0)):
        f, dev = entry[0], entry[1]
        f.row_begin, f.row_end = rows
        try:
            got = f.run_hip(ctx, dev)  # (synchronises)
        finally:
            f.row_begin, f.row_end = 0, 0
        rep = ctx.lighting_dispatch()
        assert rep["family"] == "fast"
        forms.append(rep["strays"])
        if rows == (0, 0):
            assert np.array_equal(got, want), f"call {len(forms)} ({rep['strays']}): differs from the general kernel's image"
        else:
            assert np.array_equal(got[rows[0]:rows[1]], want[rows[0]:rows[1]]) and not got[:rows[0]].any() and not got[rows[1]:].any()
        return rep["strays"]

    for _ in range(6):
        call(eb, want_b)
    call(ea, want_a)  # strays after a clean streak: finished in-kernel, once — and exact
    call(ea, want_a)
    for _ in range(6):
        call(eb, want_b)
    call(ea, want_a)
    L, I = "launch", "inline"
    assert forms == [L, L, L, L, I, I, I, L, L, L, L, L, I, I, I], forms
    # a change of the row range restarts the streak, and so does the change back
    del forms[:]
    for _ in range(5):
        call(eb, want_b)
    for _ in range(5):
        call(eb, want_b, rows=(8, 136))
    call(eb, want_b)
    assert forms == [L, L, L, L, I, L, L, L, L, I, L], forms


def test_auto_inside_a_capture_is_always_two_launches(ctx):
    import torch
    ea, eb = _frame("256x144", True, "random", 31), _frame("256x144", True, "atrium", 32)
    want_a = _want(ctx, ea)
    fb = eb[0]
    ctx.debug_set()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.set_stream(s.cuda_stream)
    try:
        dev = fb.device_arrays()  # (a copy of the atrium's arrays: its contents are replaced below)
        lits = [torch.zeros((144, 256, 4), dtype=torch.int16, device="cuda") for _ in range(2)]
        descs = [fb.describe(dev, lit) for lit in lits]
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for k in range(5):
                ctx.lighting(descs[0][0])
                s.synchronize()
        assert ctx.lighting_dispatch()["strays"] == "inline"  # the streak is clean
        forms = []
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            for d, _ in descs:
                ctx.lighting(d)
                forms.append(ctx.lighting_dispatch()["strays"])
        assert forms == ["launch", "launch"], forms
        # the same captured launches over the random frame's contents: its strays are the fix-up launch's, every time
        for k, v in ea[0].arrays.items():
            dev[k].copy_(util.to_torch(v))
        for _ in range(3):
            for lit in lits:
                lit.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            for lit in lits:
                assert np.array_equal(util.from_torch(lit, np.uint16), want_a)
        # launches the record did not count have run: what it knew has ended
        with torch.cuda.stream(s):
            ctx.lighting(descs[0][0])
            s.synchronize()
        assert ctx.lighting_dispatch()["strays"] == "launch"
        assert np.array_equal(util.from_torch(lits[0], np.uint16), want_a)
    finally:
        torch.cuda.synchronize()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
