"""Independent numpy restatement of the LPV geometry volume (include/sah_lpv_gv.h): the two injections and the propagation with
use_gv = 1, written from the shader text (gi/lpv/gv_injection.vert, inject_scene_depth_into_gv.{vert,geom}, lpv_propagate.comp.slang:104-146)
with the arithmetic model of tools/gen_golden.py (whose fma, trilinear_border and mat_vec it reuses).  It is the CPU reference of
tests/test_lpv_gv_*.py and writes the small fixtures tests/golden/lpv_gv_*.npz:

    python tools/gen_golden_gv.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import gen_golden as gg  # noqa: E402

f32, F, hf = np.float32, gg.F, np.float16
GOLDEN = gg.GOLDEN
C0, C1 = f32(0.886226925), f32(1.02332671)


# ---- the MAX blend --------------------------------------------------------------------------------------------------
def gv_key(bits):
    """order-preserving key of half bit patterns: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN"""
    b = np.asarray(bits, np.uint32)
    return np.where(b & 0x8000, (~b) & 0xFFFF, b | 0x8000).astype(np.uint32)


def gv_unkey(key):
    k = np.asarray(key, np.uint32)
    return np.where(k & 0x8000, k & 0x7FFF, (~k) & 0xFFFF).astype(np.uint16)


def blend_max(gv, cells, lobe):
    """gv (D, H, W, 4) uint16 bit patterns, modified in place; cells flat texel indices (x + W (y + H z)); lobe 4 fp32 arrays.
    Per channel dst = max(dst, RN16(src)) in the key order; a NaN source leaves its channel unchanged."""
    flat = gv.reshape(-1, 4)
    keys = gv_key(flat)
    for k in range(4):
        with np.errstate(over="ignore", invalid="ignore"):
            src = np.broadcast_to(np.asarray(lobe[k], f32), cells.shape).astype(hf)
        ok = ~np.isnan(src)
        np.maximum.at(keys[:, k], cells[ok], gv_key(src[ok].view(np.uint16)))
    flat[:] = gv_unkey(keys)
    return gv


def point_cells(ndc_x, ndc_y, layer_f, W, H, D):
    """gl_Position (ndc, 0, 1) + gl_Layer -> flat texel index, -1 when dropped (the rule of sah_lpv_inject_vpls)"""
    with np.errstate(invalid="ignore", over="ignore"):
        xf = F(F(ndc_x * f32(W * 0.5)) + f32(W * 0.5))
        yf = F(F(ndc_y * f32(H * 0.5)) + f32(H * 0.5))
        ok = (xf >= 0) & (xf < f32(W)) & (yf >= 0) & (yf < f32(H)) & (layer_f > f32(-1)) & (layer_f < f32(D))
        cx = np.where(ok, np.floor(np.where(ok, xf, 0)), 0).astype(np.int64)
        cy = np.where(ok, np.floor(np.where(ok, yf, 0)), 0).astype(np.int64)
        cz = np.where(ok, np.trunc(np.where(ok, layer_f, 0)), 0).astype(np.int64)
    return np.where(ok, cx + W * (cy + H * cz), -1)


def _outside01(cp):
    return (cp[0] < 0) | (cp[1] < 0) | (cp[2] < 0) | (cp[0] > 1) | (cp[1] > 1) | (cp[2] > 1)


def _lobe(n):
    """dir_to_cosine_lobe (spherical_harmonics.glsl:28-30) in fp32"""
    return [np.full(n[0].shape, C0, f32), F(F(-C1) * n[1]), F(C1 * n[2]), F(F(-C1) * n[0])]


def inject_rsm_gv(normals, depth, mats, first, count, num_cascades, gv):
    """gv_injection.vert for cascades [first, first + count).  normals (L, ry, rx, 4) uint8, depth (L, ry, rx) uint16, mats a ctypes array of
    LpvCascadeMatrices, gv (D, H, W, 4) uint16 modified in place."""
    ry, rx = depth.shape[1:3]
    D, H, W = gv.shape[:3]
    ident = np.eye(4, dtype=f32).reshape(16)
    for c in range(first, first + count):
        t = 2 * np.arange(rx * ry, dtype=np.int64)
        x, y = t % rx, t // rx
        keep = y < ry
        x, y = x[keep], y[keep]
        rxf, ryf = f32(rx), f32(ry)
        tu, tv = F(F(f32(0.5) + x.astype(f32)) / rxf), F(F(f32(0.5) + y.astype(f32)) / ryf)
        ix, iy = np.floor(F(tu * rxf)).astype(np.int64) % rx, np.floor(F(tv * ryf)).astype(np.int64) % ry  # NEAREST, REPEAT
        d = F(depth[c, iy, ix].astype(f32) / f32(65535))
        ndc = [F(F(F(x.astype(f32) / rxf) * f32(2)) - f32(1)), F(F(F(y.astype(f32) / ryf) * f32(2)) - f32(1))]
        with np.errstate(all="ignore"):
            vs = gg.mat_vec(ident, [ndc[0], ndc[1], d, np.ones_like(d)])
            vs = [F(v / vs[3]) for v in vs]
            ws = gg.mat_vec(np.array(mats[c].inverse_rsm_vp[:], f32), vs)
            cp = gg.mat_vec(np.array(mats[c].world_to_cascade[:], f32), ws)
        inside = ~_outside01(cp)
        n = [F(normals[c, iy, ix, k].astype(f32) / f32(255)) for k in range(3)]  # UNORM as read
        lobe = _lobe(n)
        cp = [F(v + f32(0.5 / 32)) for v in cp]
        px = F(F(cp[0] + f32(c)) / f32(num_cascades))
        cells = point_cells(F(F(px * f32(2)) - f32(1)), F(F(cp[1] * f32(2)) - f32(1)), F(cp[2] * f32(32)), W, H, D)
        cells = np.where(inside, cells, -1)
        sel = cells >= 0
        blend_max(gv, cells[sel], [v[sel] for v in lobe])
    return gv


def inject_scene_gv(depth, normals, view, mats, num_cascades, gv):
    """inject_scene_depth_into_gv.{vert,geom}.  depth (Hs, Ws) float32, normals (Hs, Ws, 4) uint16 (half bits), view an _abi.ViewData."""
    Hs, Ws = depth.shape
    D, H, W = gv.shape[:3]
    nverts = (Ws * Hs) // 4
    i = np.arange(nverts, dtype=np.int64)
    x, y = i % Ws, i // Ws
    with np.errstate(all="ignore"):
        ss = [F(F(x.astype(f32) + f32(0.5)) / f32(Ws)), F(F(y.astype(f32) + f32(0.5)) / f32(Hs))]
        vs = gg.mat_vec(np.array(view.inverse_projection[:], f32), [F(F(ss[0] * f32(2)) - f32(1)), F(F(ss[1] * f32(2)) - f32(1)), depth[y, x].astype(f32),
                                                                  np.ones(nverts, f32)])
        vs = [F(v / vs[3]) for v in vs]
        ws = gg.mat_vec(np.array(view.inverse_view[:], f32), vs)
    nb = normals[y, x, :3].astype(np.uint16).view(hf).astype(f32)
    lobe = _lobe([nb[:, 0], nb[:, 1], nb[:, 2]])
    for c in range(num_cascades):
        with np.errstate(all="ignore"):
            cp = gg.mat_vec(np.array(mats[c].world_to_cascade[:], f32), ws)
            cells = point_cells(F(F(cp[0] + f32(c)) / f32(num_cascades)), cp[1], F(cp[2] * f32(32)), W, H, D)
        cells = np.where(_outside01(cp), -1, cells)
        sel = cells >= 0
        blend_max(gv, cells[sel], [v[sel] for v in lobe])
    return gv


# ---- lpv_propagate.comp.slang with use_gv = 1 ----------------------------------------------------------------------------------------
ORIENT = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1], [-1, 0, 0, 0, 1, 0, 0, 0, -1], [0, 0, 1, 0, 1, 0, -1, 0, 0], [0, 0, -1, 0, 1, 0, 1, 0, 0],
                   [1, 0, 0, 0, 0, 1, 0, -1, 0], [1, 0, 0, 0, 0, -1, 0, 1, 0]], dtype=np.float32).reshape(6, 3, 3)
DIRS = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=np.int64)
SIDES = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], dtype=np.float32)


def _hmul33(M, v):
    M = M.astype(hf)
    return [hf(hf(hf(M[r, 0] * v[0]) + hf(M[r, 1] * v[1])) + hf(M[r, 2] * v[2])) for r in range(3)]


def _sh(d):
    return [hf(0.282094792), hf(f32(-0.488602512) * f32(d[1])), hf(f32(0.488602512) * f32(d[2])), hf(f32(-0.488602512) * f32(d[0]))]


def _cos_lobe(d):
    return [hf(0.886226925), hf(f32(-1.02332671) * f32(d[1])), hf(f32(1.02332671) * f32(d[2])), hf(f32(-1.02332671) * f32(d[0]))]


def direction_tables():
    """per neighbour n: ([(eval_sh, reproj_lobe) of the four sides], (cur_sh, cur_lobe)), half"""
    small, big = hf(0.4472135), hf(0.894427)
    out = []
    for n in range(6):
        sides = []
        for s in range(4):
            e = _hmul33(ORIENT[n], [hf(hf(SIDES[s, 0]) * small), hf(hf(SIDES[s, 1]) * small), big])
            r = _hmul33(ORIENT[n], [hf(SIDES[s, 0]), hf(SIDES[s, 1]), hf(0)])
            sides.append((_sh(e), _cos_lobe(r)))
        c = [hf(t) for t in DIRS[n]]
        out.append((sides, (_sh(c), _cos_lobe(c))))
    return out


def gv_sample(gv_bits, nx, ny, nz, cascade):
    """geo_volume.SampleLevel(((n / 32 + 0.5 / 32) + cascade) / 4, ...) -> half4 (LINEAR, CLAMP_TO_BORDER; the weighted sum in fp32)"""
    vol = gv_bits.view(hf).astype(f32)
    u = F(F(F(F(nx.astype(f32) / f32(32)) + f32(0.5 / 32)) + cascade.astype(f32)) / f32(4))
    v = F(F(ny.astype(f32) / f32(32)) + f32(0.5 / 32))
    w = F(F(nz.astype(f32) / f32(32)) + f32(0.5 / 32))
    with np.errstate(all="ignore"):
        return gg.trilinear_border(vol, u, v, w).astype(hf)


def face_factor(g, s):
    """1 - clamp(g.x * s.x + abs(dot(g.yzw, s.yzw)), 0, 1) in half; clamp = fmin(fmax(x, 0), 1): NaN -> 0"""
    with np.errstate(all="ignore"):
        d = hf(hf(hf(g[..., 1] * s[1]) + hf(g[..., 2] * s[2])) + hf(g[..., 3] * s[3]))
        t = hf(hf(g[..., 0] * s[0]) + np.abs(d))
        return hf(hf(1) - np.fmin(np.fmax(t, hf(0)), hf(1)))


def gv_factors(gv_bits, num_cascades):
    """the 30 factors of every cell: (6, 5, 32, 32, 32 * num_cascades) half; 1 where the shader skips the neighbour"""
    W = 32 * num_cascades
    tabs = direction_tables()
    zs, ys, xs = np.meshgrid(np.arange(32), np.arange(32), np.arange(W), indexing="ij")
    cx, casc = xs % 32, xs // 32
    out = np.ones((6, 5, 32, 32, W), hf)
    for n in range(6):
        dx, dy, dz = (int(t) for t in DIRS[n])
        nx, ny, nz = cx - dx, ys - dy, zs - dz
        skip = (nx > 31) | (ny > 31) | (nz > 31)
        g = gv_sample(gv_bits, nx, ny, nz, casc)
        sides, (cs, _) = tabs[n]
        for s in range(4):
            out[n, s] = np.where(skip, hf(1), face_factor(g, sides[s][0]))
        out[n, 4] = np.where(skip, hf(1), face_factor(g, cs))
    return out


def lpv_propagate_gv(vols, gv_bits, steps, num_cascades, snapshots=None):
    """lpv_propagate.comp.slang:76-156 in half with use_gv = 1 (gen_golden.lpv_propagate with the factor where it multiplies by 1).
    vols: three (32, 32, 32 * num_cascades, 4) float16 arrays; gv_bits: the GV's (D, H, W, 4) uint16 bits, or None for use_gv = 0.
    Returns the volumes after `steps` steps, or {k: volumes after k steps} for k in `snapshots`."""
    W = 32 * num_cascades
    tabs = direction_tables()
    fac = gv_factors(gv_bits, num_cascades) if gv_bits is not None else np.ones((6, 5, 32, 32, W), hf)
    direct_sa = hf(f32(hf(0.4006696846)) / f32(3.1415927))
    side_sa = hf(f32(hf(0.4234413544)) / f32(3.1415927))
    zs, ys, xs = np.meshgrid(np.arange(32), np.arange(32), np.arange(W), indexing="ij")
    cx = xs % 32
    geo = []
    for n in range(6):
        dx, dy, dz = (int(t) for t in DIRS[n])
        nx, ny, nz = cx - dx, ys - dy, zs - dz
        skip = (nx < -1) | (ny < -1) | (nz < -1) | (nx > 31) | (ny > 31) | (nz > 31)
        gx = nx + (xs - cx)
        ok = (~skip) & (gx >= 0) & (gx < W) & (ny >= 0) & (ny < 32) & (nz >= 0) & (nz < 32)
        geo.append((skip, ok, gx, ny, nz))
    cur = [v.copy() for v in vols]
    snaps = {}
    for step in range(1, steps + 1):
        nxt = []
        for vol in cur:
            acc = np.zeros((32, 32, W, 4), dtype=hf)
            for n in range(6):
                skip, ok, gx, ny, nz = geo[n]
                coef = np.zeros((32, 32, W, 4), dtype=hf)
                coef[ok] = vol[nz[ok], ny[ok], gx[ok]]
                sides, (cs, cl) = tabs[n]
                with np.errstate(all="ignore"):
                    for s, (es, rl) in enumerate(sides + [(cs, cl)]):
                        dot = hf(hf(hf(coef[..., 0] * es[0]) + hf(coef[..., 1] * es[1])) + hf(coef[..., 2] * es[2]))
                        dot = hf(dot + hf(coef[..., 3] * es[3]))
                        # max(0, x) as the library and the oracle evaluate it (IEEE maxNum: a NaN gives 0); np.maximum would keep the NaN
                        k = hf((side_sa if s < 4 else direct_sa) * np.fmax(hf(0), dot))
                        add = np.stack([hf(hf(k * rl[c]) * fac[n, s]) for c in range(4)], axis=-1)
                        acc = np.where(skip[..., None], acc, hf(acc + add))
            nxt.append(acc)
        cur = nxt
        if snapshots is not None and step in snapshots:
            snaps[step] = [v.copy() for v in cur]
    return snaps if snapshots is not None else cur


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def random_gv(rng, num_cascades, scale=0.6):
    """a GV like the injections make (lobes: x = 0.886, |yzw| <= 1.02) with holes, negatives and -0"""
    shape = (32, 32, 32 * num_cascades, 4)
    v = rng.uniform(-1.02, 1.02, shape).astype(f32) * f32(scale)
    v[..., 0] = np.where(rng.random(shape[:3]) < 0.5, f32(0.886226925), f32(0))
    v = v.astype(hf)
    v[rng.random(shape) < 0.3] = hf(0)
    v[rng.random(shape) < 0.05] = hf(-0.0)
    return np.ascontiguousarray(v.view(np.uint16))


def main():
    """lpv_gv_propagate_2c_3steps.npz: sparse light (300 cells) and a sparse GV, so that the fixture stays small"""
    rng = np.random.default_rng(2024)
    nc, steps = 2, 3
    vols = []
    for _ in range(3):
        v = np.zeros((32, 32, 32 * nc, 4), hf)
        z, y, x = rng.integers(0, 32, 300), rng.integers(0, 32, 300), rng.integers(0, 32 * nc, 300)
        v[z, y, x] = rng.uniform(-1, 1, (300, 4)).astype(hf)
        vols.append(v)
    gv = random_gv(rng, nc)
    gv[rng.random(gv.shape[:3]) < 0.9] = 0
    out = lpv_propagate_gv(vols, gv, steps, nc)
    np.savez_compressed(os.path.join(GOLDEN, "lpv_gv_propagate_2c_3steps.npz"), a=np.stack([v.view(np.uint16) for v in vols]), gv=gv,
                        b=np.stack([v.view(np.uint16) for v in out]))
    print("wrote lpv_gv_propagate_2c_3steps.npz")


if __name__ == "__main__":
    main()
