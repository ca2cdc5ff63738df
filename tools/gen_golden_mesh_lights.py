"""Independent numpy restatement of the LPV mesh lights (include/sah_lpv_mesh_lights.h): the point cloud of a mesh
(mesh_storage.cpp:246-450 with the header's pinned engine, uniform and reservoir rule), the VPLs of an emissive primitive
(emissive_point_cloud.comp) and the per-frame injection (light_propagation_volume.cpp:787-834 with vpl_injection.{vert,frag}), with the
arithmetic model of tools/gen_golden.py (whose mat_vec, sample_bias(..., explicit_lod=0) and inject_vpls it reuses).  It is the CPU
reference of tests/test_lpv_mesh_lights_*.py and writes the small fixture tests/golden/lpv_mesh_lights_atrium.npz:

    python tools/gen_golden_mesh_lights.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import gen_golden as gg  # noqa: E402
from androidrenderer_amd import _abi, mesh  # noqa: E402

f32, F = np.float32, gg.F
GOLDEN = gg.GOLDEN
FIXTURE = os.path.join(GOLDEN, "lpv_mesh_lights_atrium.npz")
ON_SURFACE, MATERIAL_ZERO = 1, 1
M31 = 2147483647


# ---- the engine and the uniform --------------------------------------------------------------------------------------------------
class MinStd0:
    """minstd_rand0 seeded the standard's way"""

    def __init__(self, seed):
        self.x = int(seed) % M31 or 1

    def __call__(self):
        self.x = self.x * 16807 % M31
        return self.x


def uniform01(e):
    """libstdc++'s generate_canonical<double, 53> over minstd_rand0: two draws, every double operation rounded"""
    R = 2147483646.0
    s = float(e() - 1) * 1.0
    s = s + float(e() - 1) * R
    ret = s / (R * R)
    return ret if ret < 1.0 else np.nextafter(1.0, 0.0)


# ---- sah_mesh_point_cloud --------------------------------------------------------------------------------------------------------
def _pack_unorm4x8(c):
    c = np.asarray(c, f32)
    with np.errstate(invalid="ignore"):
        v = np.where(c < 0, f32(0), c)
        v = np.where(f32(1) < v, f32(1), v)
        t = F(v * f32(255))
        r = np.trunc(t)
        r = r + (F(t - r) >= f32(0.5))  # std::round: halves away from zero (t >= 0 here)
    r = np.where(np.isnan(r), 0, r).astype(np.uint32)
    return r[..., 0] | (r[..., 1] << 8) | (r[..., 2] << 16) | (r[..., 3] << 24)


def point_cloud(positions, vertex_data, indices, first_index, index_count, vertex_offset, seed, flags=0):
    """-> (positions (n, 3) float32, points of mesh.VERTEX_DATA, bounds_min, bounds_max)"""
    positions = np.asarray(positions, f32).reshape(-1, 3)
    idx = np.asarray(indices, np.uint32)[first_index:first_index + index_count].astype(np.int64) + vertex_offset
    with np.errstate(invalid="ignore"):
        lo = np.fmin.reduce(positions[idx], axis=0, initial=np.inf).astype(f32) if idx.size else np.full(3, np.inf, f32)
        hi = np.fmax.reduce(positions[idx], axis=0, initial=-np.inf).astype(f32) if idx.size else np.full(3, -np.inf, f32)
    tri = idx.reshape(-1, 3)
    p = positions[tri]  # (nt, 3 corners, 3)
    with np.errstate(all="ignore"):
        a, b = F(p[:, 0] - p[:, 1]), F(p[:, 0] - p[:, 2])
        c = [F(F(a[:, 1] * b[:, 2]) - F(b[:, 1] * a[:, 2])), F(F(a[:, 2] * b[:, 0]) - F(b[:, 2] * a[:, 0])),
             F(F(a[:, 0] * b[:, 1]) - F(b[:, 0] * a[:, 1]))]
        area = gg.length3_f(c).astype(np.float64) / 2.0
        run = np.cumsum(area)  # sequential, as the reference's accumulator
        total = float(run[-1]) if run.size else 0.0
        count = int(min(np.ceil(total / 0.1), 65536.0)) if np.isfinite(total) and total > 0 else 0
        prefix = np.cumsum(area / total) if count else None
    out_p, out_v = np.zeros((count, 3), f32), np.zeros(count, mesh.VERTEX_DATA)
    if count == 0:
        return out_p, out_v, lo, hi
    e = MinStd0(seed)
    u, bc = np.zeros(count), np.zeros((count, 3), f32)
    for i in range(count):
        u[i] = uniform01(e)
        bc[i] = [f32(uniform01(e)) for _ in range(3)]
    t = np.minimum(np.searchsorted(prefix, u, side="right"), tri.shape[0] - 1)  # the first prefix > u, else the last
    with np.errstate(all="ignore"):
        inv = F(f32(1) / np.sqrt(F(F(F(bc[:, 0] * bc[:, 0]) + F(bc[:, 1] * bc[:, 1])) + F(bc[:, 2] * bc[:, 2]))))
        w = F(bc * inv[:, None])
        if flags & ON_SURFACE:
            w = F(w / F(F(w[:, 0] + w[:, 1]) + w[:, 2])[:, None])
    v = tri[t]

    def mix(attr):  # attr (N, k) per vertex -> (count, k)
        a0, a1, a2 = attr[v[:, 0]], attr[v[:, 1]], attr[v[:, 2]]
        with np.errstate(all="ignore"):
            s = F(F(F(a0 * w[:, 0:1]) + F(a1 * w[:, 1:2])) + F(a2 * w[:, 2:3]))
            return s if flags & ON_SURFACE else F(s / f32(3))
    vd = np.asarray(vertex_data)
    out_p[:] = mix(positions)
    out_v["normal"] = mix(vd["normal"].astype(f32))
    out_v["tangent"] = mix(vd["tangent"].astype(f32))
    out_v["texcoord"] = mix(vd["texcoord"].astype(f32))
    cols = np.stack([(vd["color"] >> (8 * k)) & 0xFF for k in range(4)], axis=1).astype(f32)
    out_v["color"] = _pack_unorm4x8(mix(F(cols * f32(0.0039215686274509803921568627451))))
    return out_p, out_v, lo, hi


# ---- sah_lpv_emissive_vpls ---------------------------------------------------------------------------------------------------------
def _half_bits(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, f32).astype(np.float16).view(np.uint16).astype(np.uint32)


def emissive_vpls(arrays, primitive, cloud_positions, cloud_points, flags=0):
    """(n, 4) uint32 PackedVPLs; arrays: mesh.Mesh.arrays() (host)"""
    prim = arrays["primitives"][primitive]
    mi = 0 if flags & MATERIAL_ZERO else int(prim["material"])
    n = cloud_positions.shape[0]
    color = np.zeros((n, 3), f32)
    if mi < arrays["materials"].shape[0]:
        mat = arrays["materials"][mi]
        s = np.broadcast_to(mat["emission_texel"].astype(f32), (n, 4))
        textures = arrays.get("textures") or []
        mt = arrays.get("material_textures")
        slot = int(mt[mi][3]) if textures and mt is not None and len(mt) else _abi.TEXTURE_NONE
        if slot != _abi.TEXTURE_NONE and slot < len(textures):
            uv = (cloud_points["texcoord"][:, 0].astype(f32), cloud_points["texcoord"][:, 1].astype(f32))
            s = gg.sample_bias(textures[slot], uv, None, None, 0.0, explicit_lod=0)
        with np.errstate(all="ignore"):
            color = F(s[:, :3] * mat["emission_factor"][:3].astype(f32))
    model = prim["model"].astype(f32)
    cp = cloud_positions.astype(f32)
    with np.errstate(all="ignore"):
        pos = gg.mat_vec(model, [cp[:, 0], cp[:, 1], cp[:, 2], f32(1)])
        nrm = np.fmin(np.fmax(cloud_points["normal"].astype(f32), f32(-1)), f32(1))
        sn = (np.rint(F(nrm * f32(127))).astype(np.int64) & 0xFF).astype(np.uint32)
    out = np.zeros((n, 4), np.uint32)
    out[:, 0] = _half_bits(pos[0]) | (_half_bits(pos[1]) << 16)
    out[:, 1] = _half_bits(pos[2]) | (_half_bits(color[:, 0]) << 16)
    out[:, 2] = _half_bits(color[:, 1]) | (_half_bits(color[:, 2]) << 16)
    out[:, 3] = sn[:, 0] | (sn[:, 1] << 8) | (sn[:, 2] << 16)
    return out


# ---- the injection -----------------------------------------------------------------------------------------------------------------
def inject_terms(vpls, mats, cascade, num_cascades, shape):
    """vpl_injection.{vert,frag} of gg.inject_vpls, vectorised: (cells (n,) int64, -1 when dropped; terms (n, 3, 4) float32)"""
    D, Hh, W = shape
    p = np.asarray(vpls, np.uint32).reshape(-1, 4)
    hb = lambda bits: (bits & 0xFFFF).astype(np.uint16).view(np.float16).astype(f32)
    pos = [hb(p[:, 0]), hb(p[:, 0] >> 16), hb(p[:, 1])]
    col = [hb(p[:, 1] >> 16), hb(p[:, 2]), hb(p[:, 2] >> 16)]
    sn = lambda b: np.maximum(F((b & 0xFF).astype(np.uint8).view(np.int8).astype(f32) / f32(127.0)), f32(-1.0))
    w2c = np.array(mats.world_to_cascade[:], f32)
    mixf = lambda x, y, a: F(F(x * F(f32(1) - a)) + F(y * a))
    with np.errstate(all="ignore"):
        nrm = gg.normalize3([sn(p[:, 3]), sn(p[:, 3] >> 8), sn(p[:, 3] >> 16)])
        cp = gg.mat_vec(w2c, [pos[0], pos[1], pos[2], f32(1)])
        px = F(F(cp[0] + f32(cascade)) / f32(num_cascades))
        ndc = [F(F(px * f32(2)) - f32(1)), F(F(cp[1] * f32(2)) - f32(1))]
        layer = F(cp[2] * f32(32))
        xf, yf = F(F(ndc[0] * f32(W * 0.5)) + f32(W * 0.5)), F(F(ndc[1] * f32(Hh * 0.5)) + f32(Hh * 0.5))
        keep = ~((gg.length3_f(nrm) < 1) | (gg.length3_f(col) == 0))
        keep &= (xf >= 0) & (xf < W) & (yf >= 0) & (yf < Hh) & (layer > -1) & (layer < D)
        cx = np.where(keep, np.floor(xf), 0).astype(np.int64)
        cy = np.where(keep, np.floor(yf), 0).astype(np.int64)
        cz = np.where(keep, np.trunc(layer), 0).astype(np.int64)
        sc = [F(F(c * f32(1024)) / f32(16384)) for c in col]
        Kx, Ky, Kz, Kw = f32(0), F(f32(-1) / f32(3)), F(f32(2) / f32(3)), f32(-1)
        step = lambda edge, x: np.where(x < edge, f32(0), f32(1))
        s1 = step(sc[2], sc[1])
        P = [mixf(sc[2], sc[1], s1), mixf(sc[1], sc[2], s1), mixf(Kw, Kx, s1), mixf(Kz, Ky, s1)]
        s2 = step(P[0], sc[0])
        Q = [mixf(P[0], sc[0], s2), mixf(P[1], P[1], s2), mixf(P[3], P[2], s2), mixf(sc[0], P[0], s2)]
        d = F(Q[0] - np.fmin(Q[3], Q[1]))
        e = f32(1.0e-10)
        hsv = [np.abs(F(Q[2] + F(F(Q[3] - Q[1]) / F(F(f32(6) * d) + e)))), F(d / F(Q[0] + e)), Q[0]]
        hsv[1] = F(hsv[1] * f32(2))
        K = [f32(1), F(f32(2) / f32(3)), F(f32(1) / f32(3)), f32(3)]
        corrected = []
        for k in range(3):
            t = F(hsv[0] + K[k])
            pk = np.abs(F(F(F(t - np.floor(t)) * f32(6)) - K[3]))
            corrected.append(F(hsv[2] * mixf(K[0], np.fmin(np.fmax(F(pk - K[0]), f32(0)), f32(1)), hsv[1])))
        sh = [np.full(p.shape[0], gg_c0, f32), F(F(-gg_c1) * nrm[1]), F(gg_c1 * nrm[2]), F(F(-gg_c1) * nrm[0])]
        terms = np.stack([np.stack([F(F(sh[k] * corrected[ch]) / f32(3.1415927)) for k in range(4)], axis=1) for ch in range(3)], axis=1)
    cells = np.where(keep, cx + W * (cy + Hh * cz), -1)
    return cells, terms


gg_c0, gg_c1 = f32(0.886226925), f32(1.02332671)


def accumulate(vols, cells, terms):
    """adds terms[i] onto texel cells[i] of the three volumes ((D, H, W, 4) float16, modified in place) in the order of i, one rounding
    to half per add; vectorised over cells: round r adds the r-th light of every cell"""
    keep = np.nonzero(cells >= 0)[0]
    if keep.size == 0:
        return vols
    c = cells[keep]
    order = np.argsort(c, kind="stable")
    sc = c[order]
    start = np.r_[0, np.nonzero(np.diff(sc))[0] + 1]
    rank = np.arange(sc.size) - np.repeat(start, np.diff(np.r_[start, sc.size]))
    flat = [v.reshape(-1, 4) for v in vols]
    src = terms[keep][order]
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.r_[0, np.cumsum(np.bincount(rank))]
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(len(bounds) - 1):
            sel = by_rank[bounds[r]:bounds[r + 1]]
            cells_r = sc[sel]
            for ch in range(3):
                flat[ch][cells_r] = (flat[ch][cells_r].astype(f32) + src[sel, ch]).astype(np.float16)
    return vols


def inject_vpls_fast(vpls, mats, cascade, num_cascades, vols):
    """gg.inject_vpls, vectorised (the same function: tests/test_lpv_mesh_lights_cpu.py checks it)"""
    cells, terms = inject_terms(vpls, mats, cascade, num_cascades, vols[0].shape[:3])
    return accumulate(vols, cells, terms)


def selected(arrays, cloud, bounds):
    """get_primitives_in_bounds + the emissive test; cloud: (primitive, bounds_min, bounds_max); bounds: (min_bounds, max_bounds)"""
    prim_index, lo_m, hi_m = cloud
    if prim_index >= arrays["primitives"].shape[0]:
        return False
    prim = arrays["primitives"][prim_index]
    mi = int(prim["material"])
    if int(prim["type"]) != _abi.PRIMITIVE_TYPE_SOLID or mi >= arrays["materials"].shape[0]:
        return False
    e = arrays["materials"][mi]["emission_factor"].astype(f32)
    mt = arrays.get("material_textures")
    textured = bool(arrays.get("textures")) and mt is not None and len(mt) and int(mt[mi][3]) != _abi.TEXTURE_NONE
    if not (gg.length3_f(e[:3]) > 0) and not textured:
        return False
    m = prim["model"].astype(f32)
    with np.errstate(all="ignore"):
        lo = gg.mat_vec(m, [f32(lo_m[0]), f32(lo_m[1]), f32(lo_m[2]), f32(1)])
        hi = gg.mat_vec(m, [f32(hi_m[0]), f32(hi_m[1]), f32(hi_m[2]), f32(1)])
    return all(f32(bounds[0][k]) < hi[k] and f32(bounds[1][k]) > lo[k] for k in range(3))


def inject_emissive(arrays, clouds, mats, bounds, num_cascades, vols):
    """sah_lpv_inject_emissive: clouds a list of (vpls (n, 4) uint32, primitive, bounds_min, bounds_max) in call order; mats the cascade
    matrices; bounds a list of (min_bounds, max_bounds); vols three (D, H, W, 4) float16 arrays, modified in place"""
    for c in range(num_cascades):
        lists = [v for (v, prim, lo, hi) in clouds if len(v) and selected(arrays, (prim, lo, hi), bounds[c])]
        if lists:
            inject_vpls_fast(np.concatenate(lists), mats[c], c, num_cascades, vols)
    return vols


def cascade_bounds(lpv):
    """scene.LpvCascades -> [(min_bounds, max_bounds)] per cascade (its `bounds`)"""
    return [(np.array(b.min_bounds[:], f32), np.array(b.max_bounds[:], f32)) for b in lpv.bounds]


def mesh_clouds(arrays, seed, flags=0):
    """clouds of every emissive primitive of a host mesh, numpy only: [(primitive, positions, points, bounds_min, bounds_max)] with the
    seed of mesh.emissive_clouds (seed + the ordinal of the primitive's index range)"""
    out = []
    for prim, ordinal in mesh.emissive_primitives(arrays):
        p = arrays["primitives"][prim]
        pos, pts, lo, hi = point_cloud(arrays["positions"], arrays["vertex_data"], arrays["indices"], int(p["first_index"]), int(p["index_count"]),
                                       int(p["vertex_offset"]), seed + ordinal, flags)
        out.append((prim, pos, pts, lo, hi))
    return out


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def atrium_fixture():
    """the atrium's lamp clouds (default and on-surface), their VPLs and the injection at 4 cascades from the default camera"""
    from androidrenderer_amd import scene
    arrays = mesh.atrium().arrays()
    view = scene.SceneView.default(1920, 1080)
    sun = scene.DirectionalLight()
    sun.set_direction([0.1, -1.0, -0.5])
    lpv = scene.LpvCascades()
    lpv.update_cascade_transforms(view, sun)
    out = {}
    for tag, flags in (("quirk", 0), ("surface", ON_SURFACE)):
        clouds = mesh_clouds(arrays, 1234, flags)
        vpl_clouds = [(emissive_vpls(arrays, prim, pos, pts), prim, lo, hi) for (prim, pos, pts, lo, hi) in clouds]
        vols = [np.zeros((32, 32, 128, 4), np.float16) for _ in range(3)]
        inject_emissive(arrays, vpl_clouds, lpv.matrices, cascade_bounds(lpv), 4, vols)
        out[f"{tag}_positions"] = np.concatenate([c[1] for c in clouds])
        out[f"{tag}_points"] = np.concatenate([c[2] for c in clouds]).view(np.uint8).reshape(-1, 40)
        out[f"{tag}_vpls"] = np.concatenate([v[0] for v in vpl_clouds])
        out[f"{tag}_volumes"] = np.stack(vols).view(np.uint16)
    out["primitives"] = np.array([c[0] for c in clouds], np.uint32)
    out["bounds"] = np.array([np.r_[c[3], c[4]] for c in clouds], f32)
    return out


def main():
    np.savez_compressed(FIXTURE, **atrium_fixture())
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
