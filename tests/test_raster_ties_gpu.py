"""Edges through pixel centres, on the GPU: every case of tests/raster_exact_ref.py through the four rasteriser passes, HIP == oracle ==
the exact integer reference, bit for bit.  (The conditions that give the cases their power, and oracle == exact, are checked on the CPU:
tests/test_raster_ties_cpu.py.)

A tie of an edge function is decided in four separately written places — cover() (records one lane walks), the per-pixel test of sweep()
(records a wave or the workgroup walks), sweep()'s classification of 8x8 blocks (`base + kmax < 0`: outside, `base + kmin > 0`: all in) and
tile_outside() of the binning (boxes of 16 tiles or more) — and the cases are the smallest grids that reach each of them: see
raster_exact_ref.cases().  In the shadow, G-buffer and RSM passes a fragment too many or too few shows as another depth or owner (every case
is rendered at depths z and 1 - z, so that either neighbour is the nearer one once).  The motion-vectors pass compares EQUAL against the
depth plane: a fragment too few shows as a zero vector; a fragment too many of a neighbour carries another depth and cannot show there."""
import numpy as np
import pytest

from androidrenderer_amd import _abi, images, mesh
from tests import raster_exact_ref as ex
from tests import raster_ties_util as rt

pytestmark = pytest.mark.gpu

ALL = rt.NAMES + ["same-depth"]
FORMATS = {"color": _abi.FORMAT_R8G8B8A8_SRGB, "normals": _abi.FORMAT_R16G16B16A16_SFLOAT, "data": _abi.FORMAT_R8G8B8A8_UNORM,
           "emission": _abi.FORMAT_R8G8B8A8_SRGB, "depth": _abi.FORMAT_D32_SFLOAT}


def _orders(name):
    return ("z",) if name == "same-depth" else rt.ORDERS


def _device_geometry(arrays):
    return mesh.geometry(mesh.to_device(arrays), [])


def _stats():
    import torch
    return torch.zeros(_abi.RASTER_STATS_WORDS, dtype=torch.int32, device="cuda")


def _host(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def hip_shadow(ctx, geo, cascades, W, H, pad=0):
    import torch
    sm = torch.full((cascades, H, W + pad), 0x1234, dtype=torch.int16, device="cuda")
    vol = images.volume(sm, _abi.FORMAT_D16_UNORM)
    vol.width = W
    stats = _stats()
    ctx.shadow_render(geo, rt.identity_sun(), cascades, vol, stats.data_ptr())
    torch.cuda.synchronize()
    full = _host(sm, np.uint16)
    assert (full[:, :, W:] == 0x1234).all(), "the shadow pass wrote into the padding of its rows"
    return full[:, :, :W], _host(stats, np.uint32)


def hip_gbuffer(ctx, geo, W, H, pad=0, keep_device=False):
    import torch
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    full = {k: torch.full((H, W + pad) + ((c,) if c else ()), 7, dtype=t, device="cuda") for k, (c, t) in shapes.items()}
    planes = []
    for k in ("color", "normals", "data", "emission", "depth"):
        p = images.plane(full[k], FORMATS[k])
        p.width = W
        planes.append(p)
    stats = _stats()
    ctx.gbuffer_render(geo, rt.identity_view(W, H), _abi.GBuffer(*planes), stats.data_ptr())
    torch.cuda.synchronize()
    out = {k: _host(v)[:, :W] for k, v in full.items()}
    out["normals"] = out["normals"].view(np.uint16)
    for k, v in full.items():
        assert (_host(v)[:, W:] == 7).all(), f"the G-buffer pass wrote into the padding of '{k}'"
    return (out, _host(stats, np.uint32), full) if keep_device else (out, _host(stats, np.uint32))


def hip_rsm(ctx, geo, cascades, W, H):
    import torch
    t = {"flux": torch.full((cascades, H, W, 4), 9, dtype=torch.uint8, device="cuda"), "normals": torch.full((cascades, H, W, 4), 9, dtype=torch.uint8, device="cuda"),
         "depth": torch.full((cascades, H, W), 9, dtype=torch.int16, device="cuda")}
    stats = _stats()
    ctx.rsm_render(geo, rt.identity_sun(), rt.identity_lpv(), cascades, rt.rsm_targets(t), stats.data_ptr())
    torch.cuda.synchronize()
    out = {k: _host(v) for k, v in t.items()}
    out["depth"] = out["depth"].view(np.uint16)
    return out, _host(stats, np.uint32)


def hip_motion(ctx, geo, depth, W, H, pad=0):
    """depth: the device tensor (H, W + pad) the G-buffer pass wrote"""
    import torch
    mv = torch.full((H, W + pad, 2), 0x5A5A, dtype=torch.int16, device="cuda")
    d, o = images.plane(depth, _abi.FORMAT_D32_SFLOAT), images.plane(mv, _abi.FORMAT_R16G16_SFLOAT)
    d.width = o.width = W
    stats = _stats()
    ctx.motion_vectors_render(geo, rt.identity_view(W, H, rt.MOTION_SHIFT), d, o, stats.data_ptr())
    torch.cuda.synchronize()
    full = _host(mv, np.uint16)
    assert (full[:, W:] == 0x5A5A).all(), "the motion-vectors pass wrote into the padding of its rows"
    return full[:, :W], _host(stats, np.uint32)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: HIP {got[tuple(bad[0])]}, expected {want[tuple(bad[0])]}"


def check_shadow(ctx, name, order, cascades, pad=0):
    sc, cov, own = rt.exact(name, order)
    want, want_stats = rt.oracle_shadow(name, order, cascades)
    got, got_stats = hip_shadow(ctx, _device_geometry(rt.mesh_of(name, order).arrays()), cascades, sc.W, sc.H, pad)
    _same(got, want, f"shadow cascades of {sc.name} against the oracle")
    for layer in range(cascades):
        _same(got[layer].astype(np.int64), ex.d16_code(own["rsm"][1]), f"shadow cascade {layer} of {sc.name} against the exact reference")
    assert list(got_stats[:4]) == list(want_stats[:4])
    return got_stats


def check_gbuffer(ctx, name, order, pad=0):
    sc, cov, own = rt.exact(name, order)
    want, want_stats = rt.oracle_gbuffer(name, order)
    got, got_stats = hip_gbuffer(ctx, _device_geometry(rt.mesh_of(name, order).arrays()), sc.W, sc.H, pad)
    for k in ("depth", "color", "normals", "data", "emission"):
        a, b = (got[k].view(np.uint32), want[k].view(np.uint32)) if k == "depth" else (got[k], want[k])
        _same(a, b, f"G-buffer plane '{k}' of {sc.name} against the oracle")
    _same(got["depth"].view(np.uint32), ex.depth_bits(own["gbuffer"][1]), f"G-buffer depth of {sc.name} against the exact reference")
    rt.assert_owner(got["color"], sc, own["gbuffer"][0], f"G-buffer colour of {sc.name}")
    assert list(got_stats[:4]) == list(want_stats[:4])
    return got_stats


def check_rsm(ctx, name, order, cascades=2):
    sc, cov, own = rt.exact(name, order)
    want, want_stats = rt.oracle_rsm(name, order, cascades)
    got, got_stats = hip_rsm(ctx, _device_geometry(rt.mesh_of(name, order).arrays()), cascades, sc.W, sc.H)
    for k in ("depth", "flux", "normals"):
        _same(got[k], want[k], f"RSM '{k}' of {sc.name} against the oracle")
    for layer in range(cascades):
        _same(got["depth"][layer].astype(np.int64), ex.d16_code(own["rsm"][1]), f"RSM depth layer {layer} of {sc.name} against the exact reference")
        rt.assert_owner(got["flux"][layer], sc, own["rsm"][0], f"RSM flux layer {layer} of {sc.name}")
    assert list(got_stats[:4]) == list(want_stats[:4])
    return got_stats


def check_motion(ctx, name, order, pad=0):
    sc, wins, want, depth_n = rt.motion_exact(name, order)
    geo = _device_geometry(rt.motion_mesh(name, order).arrays())
    gb, _, device = hip_gbuffer(ctx, geo, sc.W, sc.H, pad, keep_device=True)
    _same(gb["depth"].view(np.uint32), ex.depth_bits(depth_n), f"G-buffer depth of {sc.name} against the exact reference")
    got, stats = hip_motion(ctx, geo, device["depth"], sc.W, sc.H, pad)
    _same((got != 0).any(-1), wins, f"motion vectors of {sc.name}: non-zero exactly where the SOLID owner's depth is the depth texel")
    _same(got, want, f"motion vectors of {sc.name} against the fp32 restatement")
    assert wins.sum() >= 100 and (~wins).sum() >= 100 and stats[0] == len(sc.tri)  # both kinds of pixel
    return stats


@pytest.mark.parametrize("name", ALL)
def test_shadow_cascades_equal_oracle_and_exact(hip_ctx, name):
    for order in _orders(name):
        check_shadow(hip_ctx, name, order, 1)
        check_shadow(hip_ctx, name, order, 4)


@pytest.mark.parametrize("name", ALL)
def test_gbuffer_equals_oracle_and_exact(hip_ctx, name):
    for order in _orders(name):
        stats = check_gbuffer(hip_ctx, name, order)
        if name == "dense-s3":  # every tile's list is longer than 256 entries: cut into parts and merged
            assert stats[5] > 0 and stats[6] >= 1


@pytest.mark.parametrize("name", ALL)
def test_rsm_equals_oracle_and_exact(hip_ctx, name):
    for order in _orders(name):
        check_rsm(hip_ctx, name, order)


@pytest.mark.parametrize("name", rt.NAMES)
def test_motion_vectors_equal_restatement_and_exact(hip_ctx, name):
    for order in rt.ORDERS:
        check_motion(hip_ctx, name, order)


def test_dense_case_with_every_bin_list_whole_and_padded_rows(monkeypatch):
    """SAH_RASTER_MERGE_CAPACITY=0 (testing hook, read when the context is made) leaves every bin list whole: the dense case's lists of more
    than 256 entries are then walked in rounds of 256 by one workgroup.  The outputs have rows padded to an odd number of texels (the shadow
    map's pitch is then no multiple of 4: its resolve stores single texels)."""
    import torch
    from androidrenderer_amd import lib
    monkeypatch.setenv("SAH_RASTER_MERGE_CAPACITY", "0")
    ctx = lib.Context(device=0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for order in rt.ORDERS:
            for stats in (check_shadow(ctx, "dense-s3", order, 4, pad=3), check_gbuffer(ctx, "dense-s3", order, pad=5), check_rsm(ctx, "dense-s3", order),
                          check_motion(ctx, "dense-s3", order, pad=3)):
                assert stats[5] == 0 and stats[6] >= 1 and stats[4] > 4 * 256, list(stats)
    finally:
        torch.cuda.synchronize()
        ctx.close()
