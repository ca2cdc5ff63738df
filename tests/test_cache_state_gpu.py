"""The protocol of the context's derived device state (csrc/ctx_cache.hpp: the two gather copies of the Lighting pass, the keyed tables,
the grow-only scratch), pinned as traces: scripted call sequences, each on a fresh context, and after every call the point
(cache epoch, full rebuilds of the LPV gather copy, full rebuilds of the fp32 irradiance copy) — after a Lighting call also the
`table_rebuilt` word of sah_debug_lighting_dispatch.  Captured graphs (api_chain.cpp) are replayed on the strength of the epoch, so WHERE it
moves and by how much is behaviour.

The expected traces, tests/golden/cache_state_trace.json, were recorded from the library of the commit named in that file, before the state
got its one owner (tools/gen_golden_cache_state.py rewrites the file from whatever library SAH_HIP_LIBRARY names); every point is compared
for equality.  What follows from the protocol itself is asserted on its own as well, so that a bad fixture cannot hide it."""
import json
import os

import numpy as np
import pytest

from androidrenderer_amd import _abi, images, lib, mesh, synth
from tests import util

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cache_state_trace.json")
RGBA16 = _abi.FORMAT_R16G16B16A16_SFLOAT
KEYS = ("lpv_r", "lpv_g", "lpv_b")
TRACKED = _abi.GENERATION_TRACKED


class Trace:
    def __init__(self, ctx):
        self.ctx, self.points = ctx, []

    def mark(self, label, lighting=False):
        p = [label, self.ctx.cache_epoch(), *self.ctx.copy_rebuilds()]
        if lighting:
            p.append(self.ctx.lighting_dispatch()["table_rebuilt"])
        self.points.append(p)

    def light(self, label, f, dev):
        f.run_hip(self.ctx, dev)
        self.mark(label, lighting=True)

    def at(self, label):
        hits = [p for p in self.points if p[0] == label]
        assert len(hits) == 1, label
        return hits[0]


def _frame(gi, sun_mode=_abi.SHADOW_MODE_CSM, seed=71):
    return util.LightingFrame(128, 80, seed=seed, sun_mode=sun_mode, gi=gi, flavour="atrium")


def _vols(tensors):
    return [images.volume(t, RGBA16) for t in tensors]


def _zeros_like_volumes(width):
    import torch
    return [torch.zeros((32, 32, width, 4), dtype=torch.int16, device="cuda") for _ in range(3)]


def seq_lpv_callers_counter(t):
    """sah_gi::lpv_generation counted by the caller; the writers that go through the context drop the copy"""
    import torch
    ctx = t.ctx
    f = _frame(_abi.GI_LPV)
    dev = f.device_arrays()
    vols = [dev[k] for k in KEYS]
    for gen, label in ((0, "gen0"), (0, "gen0 again"), (7, "gen7"), (7, "gen7 again")):
        f.lpv_generation = gen
        t.light(label, f, dev)
    v = _vols(vols)
    ctx.lpv_clear(v[0], v[1], v[2], None, 4)
    t.mark("clear")
    t.light("gen7 after clear", f, dev)
    # one light at the origin of the list (all-zero PackedVPL words), cascade 0
    vpl = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    count = torch.ones((1,), dtype=torch.int32, device="cuda")
    ctx.lpv_inject_vpls(vpl.data_ptr(), count.data_ptr(), 1, f.lpv.matrices, 0, 4, _vols(vols))
    t.mark("inject_vpls")
    t.light("gen7 after inject_vpls", f, dev)
    arrays = mesh.atrium().arrays()
    dev_mesh, keep = mesh.to_device(arrays), []
    g = mesh.geometry(dev_mesh, keep)
    records, clouds_keep = mesh.emissive_clouds(ctx, arrays, g, 3, lib.POINT_CLOUD_ON_SURFACE)
    t.mark("emissive_vpls")
    ctx.lpv_inject_emissive(g, records, f.lpv.matrices, f.lpv.bounds, 4, _vols(vols))
    t.mark("inject_emissive")
    t.light("gen7 after inject_emissive", f, dev)
    f.lpv_generation = 9
    f.row_begin = f.row_end = 40  # a shard plan may hand a rank no rows
    t.light("gen9 empty rows", f, dev)
    f.row_begin = f.row_end = 0
    t.light("gen9 full", f, dev)
    t.light("gen9 full again", f, dev)
    torch.cuda.synchronize()


def seq_lpv_tracked(t):
    """SAH_GENERATION_TRACKED: the last propagation step writes the copy"""
    import torch
    ctx = t.ctx
    f = _frame(_abi.GI_LPV)
    dev = f.device_arrays()
    a = [dev[k] for k in KEYS]
    b = [torch.zeros_like(x) for x in a]
    f.lpv_generation = TRACKED
    dev_b = dict(dev, **dict(zip(KEYS, b)))
    ctx.lpv_propagate(_vols(a), _vols(b), 4, 1)
    t.mark("propagate")
    t.light("tracked", f, dev_b)
    ctx.lpv_propagate(_vols(a), _vols(b), 4, 1)
    t.mark("propagate again")
    t.light("tracked again", f, dev_b)
    ctx.lpv_propagate(_vols(a), _vols(b), 4, 0)
    t.mark("propagate 0 steps")
    t.light("tracked after 0 steps", f, dev_b)
    # volumes larger than the propagated cells: the last step does not emit
    a160, b160 = _zeros_like_volumes(160), _zeros_like_volumes(160)
    ctx.lpv_propagate(_vols(a160), _vols(b160), 4, 1)
    t.mark("propagate 160 wide")
    dev160 = dict(dev, **dict(zip(KEYS, b160)))
    t.light("tracked 160 wide", f, dev160)
    t.light("tracked 160 wide again", f, dev160)
    torch.cuda.synchronize()


def seq_lpv_extents(t):
    """the grow-only buffer of the copy under 4, then 3, then 4 cascades (tests/test_tracked_copies_gpu.py has the images)"""
    import torch
    ctx = t.ctx
    f4 = _frame(_abi.GI_LPV)
    dev4 = f4.device_arrays()
    t.light("4 cascades lit", f4, dev4)
    f3 = _frame(_abi.GI_LPV)
    f3.lpv_num_cascades = 3
    for k in KEYS:
        f3.arrays[k] = np.ascontiguousarray(f3.arrays[k][:, :, :96, :])
    dev3 = f3.device_arrays()
    a3 = [dev3[k] for k in KEYS]
    b3 = [torch.zeros_like(x) for x in a3]
    ctx.lpv_propagate(_vols(a3), _vols(b3), 3, 1)
    t.mark("3 cascades propagated")
    f3.lpv_generation = TRACKED
    t.light("3 cascades tracked", f3, dict(dev3, **dict(zip(KEYS, b3))))
    a4 = [dev4[k] for k in KEYS]
    b4 = [torch.zeros_like(x) for x in a4]
    ctx.lpv_propagate(_vols(a4), _vols(b4), 4, 1)
    t.mark("4 cascades propagated")
    f4.lpv_generation = TRACKED
    t.light("4 cascades tracked", f4, dict(dev4, **dict(zip(KEYS, b4))))
    torch.cuda.synchronize()


def seq_cache_gi(t):
    import torch
    ctx = t.ctx
    f = _frame(_abi.GI_CACHE, sun_mode=_abi.SHADOW_MODE_RT)
    atl, trace, ids = synth.probe_maintenance_inputs(seed=72, num_probes=1)
    atl["rtgi"] = f.arrays["probe_irr"].copy().reshape(atl["rtgi"].shape)
    atl["depth"] = f.arrays["probe_depth"].copy().reshape(atl["depth"].shape)
    atl["validity"] = f.arrays["probe_val"].copy().reshape(atl["validity"].shape)
    a_t = {k: util.to_torch(v.view(np.uint16) if v.dtype == np.float16 else v) for k, v in atl.items()}
    dev = f.device_arrays()
    dev["probe_irr"], dev["probe_depth"], dev["probe_val"] = a_t["rtgi"], a_t["depth"], a_t["validity"]
    for gen, label in ((0, "gen0"), (0, "gen0 again"), (5, "gen5"), (5, "gen5 again"), (TRACKED, "tracked"), (TRACKED, "tracked again")):
        f.probe_generation = gen
        t.light(label, f, dev)
    tr_t = util.to_torch(trace.view(np.uint16))
    ids_t = torch.from_numpy(ids.view(np.int32)).cuda()
    ctx.probe_update(util.probe_atlases_desc(a_t), images.volume(tr_t, RGBA16), ids_t.data_ptr(), 1)
    t.mark("probe_update")
    t.light("tracked after probe_update", f, dev)
    ctx.probe_notify_updated(images.volume(dev["probe_irr"], _abi.FORMAT_B10G11R11_UFLOAT_PACK32), ids_t.data_ptr(), 1)
    t.mark("probe_notify_updated")
    t.light("tracked after probe_notify_updated", f, dev)
    b_t = {k: torch.zeros_like(v) for k, v in a_t.items()}
    ctx.probe_copy(util.probe_atlases_desc(a_t), util.probe_atlases_desc(b_t), [[0.0, 0.0, 0.0]] * 4)
    t.mark("probe_copy")
    t.light("tracked after probe_copy", f, dev)
    torch.cuda.synchronize()


def _tonemap_images(w, h):
    import torch
    scene_t = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
    mips = [torch.zeros((mh, mw, 4), dtype=torch.int16, device="cuda") for (mw, mh) in images.bloom_mip_sizes(w, h, 3)]
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    return images.plane(scene_t, RGBA16), images.mipchain(mips), images.plane(out, _abi.FORMAT_R8G8B8A8_SRGB), (scene_t, mips, out)


def seq_tonemap_tables(t):
    import torch
    ctx = t.ctx
    small, large = _tonemap_images(64, 36), _tonemap_images(96, 54)
    tol = _abi.TONEMAP_TOLERANCE_1CODE
    for im, flags, label in ((small, tol, "tol 64x36"), (small, tol, "tol 64x36 again"), (large, tol, "tol 96x54"), (small, tol, "tol 64x36 back"),
                             (small, 0, "strict 64x36")):
        ctx.tonemap(im[0], im[1], im[2], flags=flags)
        t.mark(label)
    torch.cuda.synchronize()


def seq_colx_table(t):
    import torch
    f = _frame(_abi.GI_LPV)
    f.lpv_generation = 3
    dev = f.device_arrays()
    t.light("frame", f, dev)
    t.light("frame again", f, dev)
    f.view.set_render_resolution(256, 160)
    t.light("other render_resolution", f, dev)
    t.light("other render_resolution again", f, dev)
    torch.cuda.synchronize()


def seq_set_stream(t):
    import torch
    ctx = t.ctx
    f = _frame(_abi.GI_LPV)
    f.lpv_generation = 3
    dev = f.device_arrays()
    t.light("frame", f, dev)
    first = torch.cuda.current_stream()
    second = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.set_stream(second.cuda_stream)
    t.mark("second stream")
    ctx.set_stream(first.cuda_stream)
    t.mark("first stream")
    t.light("frame again", f, dev)
    torch.cuda.synchronize()


SEQUENCES = {"lpv_callers_counter": seq_lpv_callers_counter, "lpv_tracked": seq_lpv_tracked, "lpv_extents": seq_lpv_extents, "cache_gi": seq_cache_gi,
             "tonemap_tables": seq_tonemap_tables, "colx_table": seq_colx_table, "set_stream": seq_set_stream}


def record(name):
    """the trace of one sequence on a fresh context (tools/gen_golden_cache_state.py records the fixture with it)"""
    import torch
    ctx = lib.Context(0)
    try:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        t = Trace(ctx)
        t.mark("fresh context")
        SEQUENCES[name](t)
        return t
    finally:
        torch.cuda.synchronize()
        ctx.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["traces"]


@pytest.fixture(scope="module")
def traces():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = record(name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_trace_equals_the_recorded_one(traces, golden, name):
    got = traces(name).points
    for p in got:
        print(name, p)
    assert got == golden[name]


def _moved(t, before, after):
    """what a step changed: differences of (epoch, LPV rebuilds, irradiance rebuilds) between two points"""
    b, a = t.at(before), t.at(after)
    return tuple(a[i] - b[i] for i in (1, 2, 3))


def test_a_second_identical_call_moves_nothing(traces):
    for name, pairs in (("lpv_callers_counter", [("gen7", "gen7 again"), ("gen9 full", "gen9 full again")]),
                        ("lpv_tracked", [("tracked 160 wide", "tracked 160 wide again")]),
                        ("cache_gi", [("gen5", "gen5 again"), ("tracked", "tracked again")]),
                        ("tonemap_tables", [("tol 64x36", "tol 64x36 again")]),
                        ("colx_table", [("frame", "frame again"), ("other render_resolution", "other render_resolution again")])):
        t = traces(name)
        for before, after in pairs:
            assert _moved(t, before, after) == (0, 0, 0), (name, after)
            if len(t.at(after)) > 4:
                assert t.at(after)[4] == 0, (name, after)
    # with generation 0 every call rebuilds — the same launches every time: the rebuild counters move, the epoch does not
    assert _moved(traces("lpv_callers_counter"), "gen0", "gen0 again") == (0, 1, 0)
    assert _moved(traces("cache_gi"), "gen0", "gen0 again") == (0, 0, 1)


def test_clear_after_a_reusable_copy_moves_the_epoch_by_one(traces):
    assert _moved(traces("lpv_callers_counter"), "gen7 again", "clear") == (1, 0, 0)


def test_propagating_into_the_same_tracked_volumes_leaves_the_epoch(traces):
    t = traces("lpv_tracked")
    assert _moved(t, "tracked", "propagate again") == (0, 0, 0)
    assert _moved(t, "propagate again", "tracked again") == (0, 0, 0)
    assert t.at("tracked again")[2] == 0  # the Lighting pass never rebuilt the copy the propagation writes


def test_the_full_range_after_an_empty_row_range_rebuilds(traces):
    t = traces("lpv_callers_counter")
    assert _moved(t, "gen7 after inject_emissive", "gen9 empty rows")[1] == 0
    assert _moved(t, "gen9 empty rows", "gen9 full")[1] == 1


def test_set_stream_moves_nothing(traces):
    t = traces("set_stream")
    assert _moved(t, "frame", "second stream") == (0, 0, 0) and _moved(t, "second stream", "first stream") == (0, 0, 0)
    assert _moved(t, "first stream", "frame again") == (0, 0, 0) and t.at("frame again")[4] == 0
