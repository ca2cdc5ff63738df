"""LPV maintenance on pitched, offset volumes (tests/layouts.py): clear, propagation (hot and general form, at the exact extents whose last step
also emits the Lighting pass's gather copy), propagation through a geometry volume, the two geometry-volume injections, the emissive
injection, and a Lighting pass over the volumes a padded propagation left.  Bars: those of the tight tests (tests/test_post_gpu.py,
test_lpv_gv_gpu.py, test_lpv_mesh_lights_gpu.py, test_tracked_copies_gpu.py); the padded run equals the tight run bit for bit; no padding byte
changes.  The three colours, and the two sides of the ping-pong, each have a padding of their own."""
import numpy as np
import pytest

from androidrenderer_amd import _abi, images, mesh, synth
from tests import layouts, lighting_cases as lc, util
from tests.layouts import D16, D32F, NAN_FILL, RGBA8, RGBA16F, SRGBA8

pytestmark = pytest.mark.gpu

# RGBA16F volumes: base, row pitch and slice pitch multiples of 8 (csrc/api_lpv.cpp: lpv_vol_ok).  Keys: a0..a2, b0..b2 (the ping-pong's two
# sides, red / green / blue), gv.  B: no multiples of 16; slice paddings that are no multiples of the row pitch
VOLUME_LAYOUTS = {
    "A": {"a0": dict(row_pad=8, offset=8, slice_pad=8), "a1": dict(row_pad=8), "a2": dict(row_pad=8, slice_pad=8), "b0": dict(row_pad=8, offset=8),
          "b1": dict(row_pad=8, slice_pad=8, offset=16), "b2": dict(offset=8, slice_pad=8), "gv": dict(row_pad=8, offset=8, slice_pad=8)},
    "B": {"a0": dict(row_pad=24, offset=8, slice_pad=40), "a1": dict(row_pad=40, slice_pad=72), "a2": dict(row_pad=56, offset=24, slice_pad=8),
          "b0": dict(row_pad=72, slice_pad=104), "b1": dict(row_pad=88, offset=8, slice_pad=24), "b2": dict(row_pad=8, offset=40, slice_pad=56),
          "gv": dict(row_pad=104, offset=8, slice_pad=88)},
}
B_PAYLOAD = 0x3C00  # what side B holds before a propagation: every cell is overwritten


def _same(x, y):
    """bit for bit, except that a NaN is a NaN whatever its payload (the propagation's bar: test_lpv_propagate_hot_form_equals_general_form_and_oracle)"""
    xn, yn = (x & 0x7FFF) > 0x7C00, (y & 0x7FFF) > 0x7C00
    return bool(np.all((x == y) | (xn & yn)))


def _sync():
    import torch
    torch.cuda.synchronize()


def _device_volumes(a_np, spec, b_payload=B_PAYLOAD):
    """-> ([a0, a1, a2], [b0, b1, b2]) as layouts.Pitched on the device; the padding reads as NaN halves"""
    import torch
    spec = spec or {}
    a = [layouts.pitched(util.to_torch(v.copy()), RGBA16F, 3, spec.get(f"a{c}"), NAN_FILL) for c, v in enumerate(a_np)]
    b = [layouts.pitched(torch.full(v.shape, b_payload, dtype=torch.int16, device="cuda"), RGBA16F, 3, spec.get(f"b{c}"), NAN_FILL) for c, v in enumerate(a_np)]
    return a, b


def _nonfinite_volumes(nc):
    """the `nonfinite` contents of test_lpv_propagate_hot_form_equals_general_form_and_oracle"""
    rng = np.random.default_rng(72)
    d, h, w = 32, 32, 32 * nc
    vols = []
    for c in range(3):
        kind = rng.integers(0, 8, (d, h, w, 4))
        v = rng.uniform(-2.0, 2.0, (d, h, w, 4)).astype(np.float16)
        v = np.where(kind == 0, np.float16(0.0), v)
        v = np.where(kind == 1, np.float16(-0.0), v)
        v = np.where(kind == 2, (rng.uniform(-1, 1, v.shape) * 6.0e-6).astype(np.float16), v)
        v = np.where(kind == 3, (rng.choice([-1.0, 1.0], v.shape) * rng.uniform(3.0e4, 65504.0, v.shape)).astype(np.float16), v)
        v = np.where(kind == 4, np.float16(0.5), v)
        v = np.where(kind == 5, np.float16(-0.5), v)
        zz, yy, xx = rng.integers(0, d, 40), rng.integers(0, h, 40), rng.integers(0, w, 40)
        v[zz[:15], yy[:15], xx[:15], 0] = np.float16(np.inf)
        v[zz[15:30], yy[15:30], xx[15:30], 2] = np.float16(-np.inf)
        v[zz[30:], yy[30:], xx[30:], 3] = np.float16(np.nan)
        vols.append(np.ascontiguousarray(v).view(np.uint16))
    return vols


def _oracle_propagate(a_np, nc, steps):
    a = [v.copy() for v in a_np]
    b = [np.full_like(v, B_PAYLOAD) for v in a]
    av = (_abi.Volume * 3)(*[images.volume(v, RGBA16F) for v in a])
    bv = (_abi.Volume * 3)(*[images.volume(v, RGBA16F) for v in b])
    assert util.oracle().orc_lpv_propagate(av, bv, nc, steps) == 0
    return a + b


def _hip_propagate(ctx, a_np, nc, steps, spec, gv=None):
    a, b = _device_volumes(a_np, spec)
    if gv is None:
        ctx.lpv_propagate([p.volume() for p in a], [p.volume() for p in b], nc, steps)
    else:
        ctx.lpv_propagate_gv([p.volume() for p in a], [p.volume() for p in b], gv.volume(), nc, steps)
    _sync()
    layouts.assert_padding_intact(a, b, what="lpv_propagate")
    if gv is not None:
        layouts.assert_padding_intact(gv, what="lpv_propagate_gv")
        layouts.assert_inputs_unchanged(gv, what="lpv_propagate_gv")
    return [p.read(np.uint16) for p in a + b], a, b


def _check_propagate(ctx, a_np, nc, steps, layout):
    want = _oracle_propagate(a_np, nc, steps)
    for force_general in (False, True):
        ctx.debug_set(force_general=force_general)
        try:
            tight, _, _ = _hip_propagate(ctx, a_np, nc, steps, None)
            got, _, _ = _hip_propagate(ctx, a_np, nc, steps, VOLUME_LAYOUTS[layout])
        finally:
            ctx.debug_set(force_general=False)
        form = "general" if force_general else "hot"
        for i in range(6):
            assert _same(got[i], want[i]), f"{form} form, volume {i}: {int((got[i] != want[i]).sum())} halves differ from the oracle"
            assert np.array_equal(got[i], tight[i]), f"{form} form, volume {i}: the padded run differs from the tight run"


@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("steps", [1, 4])
@pytest.mark.parametrize("nc", [3, 4])
def test_lpv_propagate_on_pitched_volumes(hip_ctx, nc, steps, layout):
    """volumes of exactly (32 nc) x 32 x 32 — the extent at which the last step also emits the gather copy — with row and slice pitches larger
    than the payload: the hot form walks neighbours by adding the pitches to a 32-bit offset, per colour volume"""
    a_np = [v.view(np.uint16).copy() for v in synth.lpv_volumes(nc, seed=31)]
    _check_propagate(hip_ctx, a_np, nc, steps, layout)


def test_lpv_propagate_nonfinite_contents_on_pitched_volumes(hip_ctx):
    """waves that hold an inf / NaN leave the hot form: the general form's addressing in the same launch"""
    _check_propagate(hip_ctx, _nonfinite_volumes(4), 4, 3, "B")


@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("nc", [3, 4])
def test_lpv_clear_on_pitched_volumes(hip_ctx, nc, layout):
    a_np = [v.view(np.uint16).copy() for v in synth.lpv_volumes(nc, seed=32)]
    spec = VOLUME_LAYOUTS[layout]
    a, _ = _device_volumes(a_np, spec)
    gv = layouts.pitched(util.to_torch(a_np[0].copy()), RGBA16F, 3, spec["gv"], NAN_FILL)
    hip_ctx.lpv_clear(a[0].volume(), a[1].volume(), a[2].volume(), gv.volume(), nc)
    _sync()
    layouts.assert_padding_intact(a, gv, what="lpv_clear")
    for p in a + [gv]:
        assert not p.read(np.uint16).any()
    # a volume wider than the cascades cleared: the oracle's clear on tight arrays says which cells stay
    wide = [np.full((33, 34, 32 * nc + 5, 4), 0x3C00, np.uint16) for _ in range(4)]
    want = [v.copy() for v in wide]
    vs = [images.volume(v, RGBA16F) for v in want]
    import ctypes as C
    assert util.oracle().orc_lpv_clear(C.byref(vs[0]), C.byref(vs[1]), C.byref(vs[2]), C.byref(vs[3]), nc) == 0
    dev = [layouts.pitched(util.to_torch(v), RGBA16F, 3, spec[k], NAN_FILL) for v, k in zip(wide, ("a0", "a1", "a2", "gv"))]
    hip_ctx.lpv_clear(*[p.volume() for p in dev], nc)
    _sync()
    layouts.assert_padding_intact(dev, what="lpv_clear")
    for p, w in zip(dev, want):
        assert np.array_equal(p.read(np.uint16), w)


# ---- the geometry volume ------------------------------------------------------------------------------------------------------------------

def _ggv():
    from tests.test_lpv_gv_gpu import ggv
    return ggv


@pytest.mark.parametrize("layout", ["A", "B"])
def test_lpv_propagate_gv_on_pitched_volumes(hip_ctx, layout):
    ggv = _ggv()
    nc = 3
    rng = np.random.default_rng(30 + nc)
    vols = [rng.uniform(-1, 1, (32, 32, 32 * nc, 4)).astype(np.float16) for _ in range(3)]
    gv_np = ggv.random_gv(rng, nc)
    want = ggv.lpv_propagate_gv(vols, gv_np, 3, nc)
    a_np = [v.view(np.uint16) for v in vols]
    spec = VOLUME_LAYOUTS[layout]
    tight, _, _ = _hip_propagate(hip_ctx, a_np, nc, 3, None, gv=layouts.pitched(util.to_torch(gv_np), RGBA16F, 3, None, NAN_FILL))
    got, _, _ = _hip_propagate(hip_ctx, a_np, nc, 3, spec, gv=layouts.pitched(util.to_torch(gv_np), RGBA16F, 3, spec["gv"], NAN_FILL))
    for c in range(3):  # three steps: the result is in B
        ref = want[c].view(np.uint16)
        assert np.array_equal(got[3 + c], ref), f"colour {c}: {int((got[3 + c] != ref).sum())} halves differ"
    for i in range(6):
        assert np.array_equal(got[i], tight[i]), i


RSM_RES = 128
RSM_LAYOUTS = {"A": {"normals": dict(row_pad=4, offset=4, slice_pad=4), "depth": dict(row_pad=2, offset=2, slice_pad=2)},
               "B": {"normals": dict(row_pad=20, slice_pad=36), "depth": dict(row_pad=6, offset=4, slice_pad=50)}}
PLANE_LAYOUTS = {"A": {"depth": dict(row_pad=4, offset=4), "normals": dict(row_pad=8, offset=8)},
                 "B": {"depth": dict(row_pad=20), "normals": dict(row_pad=40, offset=24)}}
_gv_inputs = {}


def _gv_case(ctx):
    """the library's own RSM and G-buffer of the atrium (as the tight tests of test_lpv_gv_gpu.py make them), once per session, on the host"""
    if not _gv_inputs:
        import torch
        from tests.test_lpv_inject import _hip_rsm, _setup
        W, H = 333, 187
        view, sun, lpv = _setup(W, H)
        rsm = _hip_rsm(ctx, mesh.atrium().arrays(), sun, lpv)
        dev = mesh.to_device(mesh.atrium(2).arrays())
        g = mesh.geometry(dev, [])
        shapes = {"color": ((H, W, 4), torch.uint8), "normals": ((H, W, 4), torch.int16), "data": ((H, W, 4), torch.uint8),
                  "emission": ((H, W, 4), torch.uint8), "depth": ((H, W), torch.float32)}
        gb = {k: torch.zeros(s, dtype=t, device="cuda") for k, (s, t) in shapes.items()}
        ctx.gbuffer_render(g, view.gpu_data, images.gbuffer(gb))
        _sync()
        _gv_inputs.update(view=view, lpv=lpv, rsm_normals=util.from_torch(rsm["normals"], np.uint8).reshape(4, RSM_RES, RSM_RES, 4),
                          rsm_depth=util.from_torch(rsm["depth"], np.uint16).reshape(4, RSM_RES, RSM_RES),
                          depth=util.from_torch(gb["depth"], np.float32).reshape(H, W), normals=util.from_torch(gb["normals"], np.uint16).reshape(H, W, 4))
    return _gv_inputs


def _prior_gv():
    from tests.test_lpv_gv_gpu import _prior
    return _prior("random", 4, 7)


@pytest.mark.parametrize("layout", ["A", "B"])
def test_lpv_inject_rsm_gv_on_pitched_images(hip_ctx, layout):
    import torch
    ggv, c = _ggv(), _gv_case(hip_ctx)
    gv0 = _prior_gv()
    want = ggv.inject_rsm_gv(c["rsm_normals"], c["rsm_depth"], c["lpv"].matrices, 0, 4, 4, gv0.copy())
    assert (want != gv0).any()
    results = []
    for rs, gs in ((None, None), (RSM_LAYOUTS[layout], VOLUME_LAYOUTS[layout]["gv"])):
        rs = rs or {}
        n = layouts.pitched(util.to_torch(c["rsm_normals"]), RGBA8, 3, rs.get("normals"))
        d = layouts.pitched(util.to_torch(c["rsm_depth"]), D16, 3, rs.get("depth"))
        flux = torch.zeros((4, RSM_RES, RSM_RES, 4), dtype=torch.uint8, device="cuda")  # (not read by the injection)
        gv = layouts.pitched(util.to_torch(gv0.copy()), RGBA16F, 3, gs, NAN_FILL)
        hip_ctx.lpv_inject_rsm_gv(_abi.RsmTargets(images.volume(flux, SRGBA8), n.volume(), d.volume()), c["lpv"].matrices, 0, 4, 4, gv.volume())
        _sync()
        layouts.assert_padding_intact(n, d, gv, what="lpv_inject_rsm_gv")
        layouts.assert_inputs_unchanged(n, d, what="lpv_inject_rsm_gv")
        results.append(gv.read(np.uint16))
    assert np.array_equal(results[1], want), f"{int((results[1] != want).sum())} halves differ"
    assert np.array_equal(results[1], results[0])


@pytest.mark.parametrize("layout", ["A", "B"])
def test_lpv_inject_scene_gv_on_pitched_images(hip_ctx, layout):
    ggv, c = _ggv(), _gv_case(hip_ctx)
    gv0 = _prior_gv()
    want = ggv.inject_scene_gv(c["depth"], c["normals"], c["view"].gpu_data, c["lpv"].matrices, 4, gv0.copy())
    assert (want != gv0).any()
    results = []
    for ps, gs in ((None, None), (PLANE_LAYOUTS[layout], VOLUME_LAYOUTS[layout]["gv"])):
        ps = ps or {}
        depth = layouts.pitched(util.to_torch(c["depth"]), D32F, 2, ps.get("depth"), NAN_FILL)
        normals = layouts.pitched(util.to_torch(c["normals"]), RGBA16F, 2, ps.get("normals"), NAN_FILL)
        gv = layouts.pitched(util.to_torch(gv0.copy()), RGBA16F, 3, gs, NAN_FILL)
        hip_ctx.lpv_inject_scene_gv(depth.plane(), normals.plane(), c["view"].gpu_data, c["lpv"].matrices, 4, gv.volume())
        _sync()
        layouts.assert_padding_intact(depth, normals, gv, what="lpv_inject_scene_gv")
        layouts.assert_inputs_unchanged(depth, normals, what="lpv_inject_scene_gv")
        results.append(gv.read(np.uint16))
    assert np.array_equal(results[1], want), f"{int((results[1] != want).sum())} halves differ"
    assert np.array_equal(results[1], results[0])


# ---- mesh lights ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("case", ["atrium", "soup"])  # the single-workgroup and the multi-workgroup form of the injection
def test_lpv_inject_emissive_into_pitched_volumes(hip_ctx, case, layout):
    from tests import test_lpv_mesh_lights_gpu as ml
    arrays = mesh.atrium().arrays() if case == "atrium" else ml._soup()
    view, sun, lpv = ml._lpv(1920, 1080) if case == "atrium" else ml._lpv()
    g, records, host, keep = ml._clouds(hip_ctx, arrays, 1234 if case == "atrium" else 5, 0)
    assert (sum(r.count for r in records) * 4 <= 4096) == (case == "atrium")
    prior = [np.random.default_rng(90 + c).uniform(-1, 1, ml.SHAPE).astype(np.float16).view(np.uint16) for c in range(3)]  # onto filled volumes
    want = ml._want(arrays, host, lpv, prior)
    assert any((w != p).any() for w, p in zip(want, prior))
    results = []
    for spec in (None, VOLUME_LAYOUTS[layout]):
        a, _ = _device_volumes(prior, spec)
        hip_ctx.lpv_inject_emissive(g, records, lpv.matrices, lpv.bounds, 4, [p.volume() for p in a])
        _sync()
        layouts.assert_padding_intact(a, what="lpv_inject_emissive")
        results.append([p.read(np.uint16) for p in a])
    for c in range(3):
        assert np.array_equal(results[1][c], want[c]), f"colour {c}: {int((results[1][c] != want[c]).sum())} halves differ"
        assert np.array_equal(results[1][c], results[0][c]), c


# ---- the gather copy a padded propagation emits -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [1, 4])
@pytest.mark.parametrize("nc", [3, 4])
def test_lighting_gathers_from_the_copy_a_padded_propagation_emitted(nc, steps):
    """tests/test_tracked_copies_gpu.py's chain with padded volumes: sah_lpv_propagate over exact-extent volumes whose pitches are larger than
    their payload, then sah_lighting over the volumes the last step stored, the generation tracked — the oracle's image, from the copy the
    step emitted (no rebuild).  The three colours of a side share one layout here (the fast Lighting path asks for that: csrc/api.cpp,
    fast_lpv_ok); the two sides differ."""
    import torch
    from androidrenderer_amd import lib
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        keys = ("lpv_r", "lpv_g", "lpv_b")
        f = lc.MatrixFrame(160, 96, seed=61, flavour="atrium", lpv=dict(num_cascades=nc), **lc.CSM_LPV)
        a_np = [f.arrays[k].view(np.uint16).copy() for k in keys]
        final_np = _oracle_propagate(a_np, nc, steps)
        final_np = final_np[3:] if steps & 1 else final_np[:3]
        side_a, side_b = dict(row_pad=24, offset=8, slice_pad=40), dict(row_pad=8, slice_pad=56, offset=16)
        a, b = _device_volumes(a_np, {f"a{c}": side_a for c in range(3)} | {f"b{c}": side_b for c in range(3)})
        ctx.lpv_propagate([p.volume() for p in a], [p.volume() for p in b], nc, steps)
        final = b if steps & 1 else a
        for k, ref in zip(keys, final_np):
            f.arrays[k] = ref.view(np.float16)
        want = f.run_oracle()
        dev = f.device_arrays()
        for k, p, ref in zip(keys, final, final_np):
            assert np.array_equal(p.read(np.uint16), ref), k
            dev[k] = p  # the very volumes the propagation stored
        f.lpv_generation = _abi.GENERATION_TRACKED
        got = f.run_hip(ctx, dev)
        rep = ctx.lighting_dispatch()
        assert rep["family"] == "fast", rep
        assert ctx.copy_rebuilds()[0] == 0, "the Lighting pass rebuilt the gather copy although the propagation had just written it"
        assert int(util.f16_ulp_diff(got, want).max()) == 0  # test_lighting_gathers_from_the_copy_the_last_propagation_step_wrote's bar
        layouts.assert_padding_intact(a, b, what="lpv_propagate + lighting")
        f.lpv_generation = 0  # a full rebuild from the padded volumes: the same image
        rebuilt = f.run_hip(ctx, dev)
        assert ctx.copy_rebuilds()[0] == 1 and np.array_equal(rebuilt, got)
    finally:
        torch.cuda.synchronize()
        ctx.close()
