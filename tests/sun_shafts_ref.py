"""The arithmetic of include/sah_sun_shafts.h restated in numpy: fp32, every operator rounded on its own, vectorised over the march texels
with a loop over the samples.  sun_shafts_ex() returns `out` and everything a test wants to look at; the scene helpers below build the
small views, suns and shadow maps the tests and tools/gen_golden_sun_shafts.py share."""
import numpy as np

from tests import ssr_ref

f32 = np.float32
DITHER, TERM_ONLY = 1, 2
MAX_STEPS = 64
BAYER = ssr_ref.BAYER.reshape(4, 4).astype(np.uint32)  # sah_ssr.h's matrix, the one the passes share
INV_4PI = f32(0.07957747)
DEFAULTS = dict(step_length=0.5, num_steps=32, step_transmittance=0.98, albedo=(1.0, 1.0, 1.0), ambient=(0.0, 0.0, 0.0), anisotropy=0.6,
                depth_bias=0.0005, depth_sharpness=50.0, downscale=1, dither_offset=0, flags=0)


def h2f(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(f32)


def to_half_bits(v):
    """half(v) of the header: round to nearest even, a NaN stored as 0x7E00"""
    v = np.asarray(v, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = v.astype(np.float16).view(np.uint16).copy()
    h[np.isnan(v)] = 0x7E00
    return h


def clamp01(a):
    with np.errstate(invalid="ignore"):
        return np.where(a > 0, np.where(a < 1, a, f32(1.0)), f32(0.0)).astype(f32)


def mul44(m, x, y, z, w):
    m = np.asarray(m, f32)
    return [((m[i] * x + m[4 + i] * y) + m[8 + i] * z) + m[12 + i] * w for i in range(4)]


def biased_matrix(M):
    """biasMat * cascade_matrices[c] as sah_lighting forms it (column major)"""
    M = np.asarray(M, f32)
    o, h, z = f32(1.0), f32(0.5), f32(0.0)
    out = np.zeros(16, f32)
    for col in range(4):
        m = M[col * 4:col * 4 + 4]
        out[col * 4 + 0] = ((h * m[0] + z * m[1]) + z * m[2]) + h * m[3]
        out[col * 4 + 1] = ((z * m[0] + h * m[1]) + z * m[2]) + h * m[3]
        out[col * 4 + 2] = ((z * m[0] + z * m[1]) + o * m[2]) + z * m[3]
        out[col * 4 + 3] = ((z * m[0] + z * m[1]) + z * m[2]) + o * m[3]
    return out


def step_table(tau, num_steps):
    P, D = f32(1.0), np.zeros(num_steps, f32)
    for k in range(num_steps):
        nxt = f32(P * f32(tau))
        D[k] = P - nxt
        P = nxt
    return D


def shadow_pcf(sm, layer, u, v, ref):
    """Lighting's bilinear compare (lighting_common.hpp: shadow_pcf) at the lanes given; sm (layers, H, W) uint16 or float32"""
    H, W = sm.shape[1:]
    px, py = u * f32(W) - f32(0.5), v * f32(H) - f32(0.5)
    fx0, fy0 = np.floor(px), np.floor(py)
    fx, fy = px - fx0, py - fy0
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    xs = [np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)]
    ys = [np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)]
    wx0, wy0 = f32(1.0) - fx, f32(1.0) - fy
    weights = [wx0 * wy0, fx * wy0, wx0 * fy, fx * fy]
    r = np.zeros(u.shape, f32)
    for k in range(4):
        d = sm[layer, ys[k >> 1], xs[k & 1]]
        if sm.dtype == np.uint16:
            d = d.astype(f32) / f32(65535.0)
        r = r + weights[k] * (ref < d).astype(f32)
    return r


def dither(mx, my, dither_offset, flags):
    """Dither of the header: the offset o of march texel (mx, my) inside its step"""
    if flags & DITHER:
        return (((BAYER[my & 3, mx & 3] + np.uint32(dither_offset)) & 15).astype(f32) + f32(0.5)) * f32(0.0625)
    return np.full(np.shape(mx), 0.5, f32)


def _params(settings):
    p = dict(DEFAULTS)
    unknown = set(settings) - set(p)
    assert not unknown, unknown
    p.update(settings)
    return p


def _d_min(z_near, p):
    return f32(z_near) / (f32(p["step_length"]) * f32(p["num_steps"]))


def march(view, sun, shadowmap, depth, **settings):
    """the march plane: -> dict with S (mh, mw, 3), T, E, V, ph, L (fp32, before the rounding to halfs) and bits (mh, mw, 4) uint16"""
    p = _params(settings)
    s, steps = int(p["downscale"]), int(p["num_steps"])
    depth = np.asarray(depth, f32)
    h, w = depth.shape
    sl = f32(p["step_length"])
    D = step_table(p["step_transmittance"], steps)
    d_min = _d_min(view.z_near, p)
    inv_view, inv_proj, vm = (np.array(m[:], f32) for m in (view.inverse_view, view.inverse_projection, view.view))
    n = -np.array(sun.direction_and_tan_size[0:3], f32)
    inv = f32(1.0) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    l = n * inv
    lv = [(vm[r] * l[0] + vm[4 + r] * l[1]) + vm[8 + r] * l[2] for r in range(3)]
    z0, o1 = f32(0.0), f32(1.0)
    A = mul44(inv_view, z0, z0, z0, o1)
    biased = [biased_matrix(sun.cascade_matrices[c][:]) for c in range(4)]
    a = []
    for c in range(4):
        ac = mul44(biased[c], A[0], A[1], A[2], o1)
        a.append([ac[i] / ac[3] for i in range(3)])
    splits = [f32(sun.data[i][0]) for i in range(4)]
    g = f32(p["anisotropy"])
    g1, g2, g3 = o1 + g * g, o1 - g * g, f32(2.0) * g
    num_cascades = 0 if shadowmap is None else min(shadowmap.shape[0], 4)

    my, mx = np.meshgrid(np.arange((h + s - 1) // s), np.arange((w + s - 1) // s), indexing="ij")
    x, y = mx * s, my * s
    with np.errstate(all="ignore"):
        d = depth[y, x]
        d = np.where(d > d_min, d, d_min).astype(f32)
        tx, ty = (x.astype(f32) + f32(0.5)) / f32(w), (y.astype(f32) + f32(0.5)) / f32(h)
        v = mul44(inv_proj, tx * f32(2.0) - o1, ty * f32(2.0) - o1, d, o1)
        ex, ey, ez = v[0] / v[3], v[1] / v[3], v[2] / v[3]
        L = np.sqrt((ex * ex + ey * ey) + ez * ez)
        B = mul44(inv_view, ex, ey, ez, o1)
        delta = []
        for c in range(4):
            b = mul44(biased[c], B[0], B[1], B[2], B[3])
            delta.append([b[i] / b[3] - a[c][i] for i in range(3)])
        nn, r = L / sl, sl / L
        o = dither(mx, my, p["dither_offset"], p["flags"])
        E, V = np.zeros(mx.shape, f32), np.zeros(mx.shape, f32)
        samples = taps = 0
        for k in range(steps):
            kf = f32(k)
            frac = clamp01(nn - kf)
            if not (frac > 0).any():
                break
            t = (kf + o * frac) * r
            zv = ez * t
            cas = np.zeros(mx.shape, np.int64)
            for i in range(4):
                cas = np.where(zv < splits[i], i + 1, cas)
            vis = np.ones(mx.shape, f32)
            if shadowmap is not None:
                c = np.minimum(cas, 3)
                sel = lambda vals: np.choose(c, vals)  # noqa: E731
                sp = [sel([np.broadcast_to(a[q][i], mx.shape) for q in range(4)]) + sel([delta[q][i] for q in range(4)]) * t for i in range(3)]
                inside = (sp[0] >= 0) & (sp[0] <= 1) & (sp[1] >= 0) & (sp[1] <= 1) & (sp[2] >= 0) & (sp[2] <= 1)
                need = (frac > 0) & (cas < num_cascades) & inside
                if need.any():
                    ref = sp[2][need] - f32(p["depth_bias"])
                    if shadowmap.dtype == np.uint16:
                        ref = np.where(ref < 0, f32(0.0), np.where(ref > 1, f32(1.0), ref)).astype(f32)
                    vis[need] = shadow_pcf(shadowmap, cas[need], sp[0][need], sp[1][need], ref)
                taps += int(need.sum())
            samples += int((frac > 0).sum())
            E = E + frac * D[k]
            V = V + (vis * frac) * D[k]
        c = ((ex / L) * lv[0] + (ey / L) * lv[1]) + (ez / L) * lv[2]
        q = g1 - g3 * c
        ph = (g2 / (q * np.sqrt(q))) * INV_4PI
        T = o1 - E
        S = np.stack([E * f32(p["ambient"][ch]) + (ph * f32(sun.color[ch])) * (f32(p["albedo"][ch]) * V) for ch in range(3)], -1).astype(f32)
    bits = np.concatenate([to_half_bits(S), to_half_bits(T)[..., None]], -1)
    return dict(S=S, T=T.astype(f32), E=E, V=V, ph=ph.astype(f32), L=L.astype(f32), bits=bits, D=D, samples=samples, taps=taps, d_min=d_min)


def upsample_weights(depth, z_near, d_min, depth_sharpness, mw, mh):
    """Composite of the header under downscale 2: -> (X (2, w), Y (2, h), W (4, h, w)) the four texels of every pixel and their weights"""
    h, w = depth.shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    X = [x >> 1, np.minimum((x >> 1) + 1, mw - 1)]
    Y = [y >> 1, np.minimum((y >> 1) + 1, mh - 1)]
    fx, fy = np.where(x & 1, f32(0.5), f32(0.0)).astype(f32), np.where(y & 1, f32(0.5), f32(0.0)).astype(f32)
    gx, gy = f32(1.0) - fx, f32(1.0) - fy
    bw = [gx * gy, fx * gy, gx * fy, fx * fy]
    with np.errstate(all="ignore"):
        d_eff = np.where(depth > d_min, depth, d_min).astype(f32)
        z = f32(z_near) / d_eff
        W = []
        for j in range(4):
            zj = z[2 * Y[j >> 1], 2 * X[j & 1]]
            W.append(bw[j] * (f32(1.0) / (f32(1.0) + (f32(depth_sharpness) * np.abs(z - zj)) / z)))
    return X, Y, W


def composite(march_bits, depth, lit_bits, z_near, **settings):
    """`out` from the stored march plane: (h, w, 4) uint16"""
    p = _params(settings)
    depth = np.asarray(depth, f32)
    h, w = depth.shape
    st = h2f(march_bits)
    with np.errstate(all="ignore"):
        if p["downscale"] == 1:
            term, term_bits = st, march_bits
        else:
            mh, mw = march_bits.shape[:2]
            X, Y, W = upsample_weights(depth, z_near, _d_min(z_near, p), p["depth_sharpness"], mw, mh)
            total = ((W[0] + W[1]) + W[2]) + W[3]
            t = [st[Y[j >> 1], X[j & 1]] for j in range(4)]
            term = ((((W[0][..., None] * t[0] + W[1][..., None] * t[1]) + W[2][..., None] * t[2]) + W[3][..., None] * t[3]) / total[..., None]).astype(f32)
            term_bits = to_half_bits(term)
        if p["flags"] & TERM_ONLY:
            return term_bits.copy()
        lit_bits = np.asarray(lit_bits, np.uint16)
        lit = h2f(lit_bits[..., :3])
        o = lit * term[..., 3:4] + term[..., :3]
        identity = (term[..., 3] == 1) & (term[..., :3] == 0).all(-1)
        finite = (np.abs(o) < np.inf).all(-1)
        out = lit_bits.copy()
        write = ~identity & finite
        out[..., :3][write] = to_half_bits(o)[write]
    return out


def sun_shafts_ex(view, sun, shadowmap, depth, lit_bits, **settings):
    info = march(view, sun, shadowmap, depth, **settings)
    return composite(info["bits"], depth, lit_bits, view.z_near, **settings), info


def sun_shafts(view, sun, shadowmap, depth, lit_bits, **settings):
    return sun_shafts_ex(view, sun, shadowmap, depth, lit_bits, **settings)[0]


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def scene_view(w, h, yaw_degrees=90.0, position=(-7.0, 1.0, 0.0), pitch_degrees=0.0):
    """a camera in the atrium (androidrenderer_amd.scene.SceneView): -> the view object; .gpu_data is the sah_view_data"""
    import math
    from androidrenderer_amd import scene
    v = scene.SceneView()
    v.rotate(math.radians(pitch_degrees), math.radians(yaw_degrees))
    v.set_position(list(position))
    v.set_render_resolution(w, h)
    v.set_perspective_projection(75.0, float(w) / float(h), 0.05)
    v.update_transforms()
    return v


def scene_sun(view, direction=(0.1, -1.0, -1.0), color=(80000.0, 80000.0, 80000.0), resolution=64, max_shadow_distance=32.0):
    """a sun with its four cascades fitted to `view`: -> sah_sun_light_constants"""
    from androidrenderer_amd import _abi, scene
    sun = scene.DirectionalLight(shadow_mode=_abi.SHADOW_MODE_CSM)
    sun.set_direction(list(direction))
    sun.set_color(list(color) + [0.0])
    sun.update_shadow_cascades(view, resolution=resolution, max_shadow_distance=max_shadow_distance)
    return sun.constants


def noise_map(layers, resolution, seed, dtype=np.uint16, lo=0.3, hi=0.7, block=1):
    """a shadow map of blocky noise in [lo, hi]: every compare outcome and every weight occur"""
    g = np.random.default_rng(seed)
    cells = (resolution + block - 1) // block
    v = g.uniform(lo, hi, (layers, cells, cells)).repeat(block, 1).repeat(block, 2)[:, :resolution, :resolution]
    if dtype == np.uint16:
        return np.round(v * 65535.0).astype(np.uint16)
    return v.astype(f32)


def constant_map(layers, resolution, value, dtype=np.uint16):
    return np.full((layers, resolution, resolution), value, dtype)


def box_depth(w, h, near=0.2, far=0.004, seed=0, holes=True):
    """reversed-Z depth: a far wall, a near box in the middle and, with `holes`, sky texels"""
    d = np.full((h, w), far, f32)
    d[h // 4:3 * h // 4, w // 3:2 * w // 3] = near
    if holes:
        g = np.random.default_rng(seed)
        d[g.random((h, w)) < 0.08] = 0.0
    return d


def textured_lit(w, h, seed):
    g = np.random.default_rng(seed)
    v = g.uniform(0.0, 4.0, (h, w, 4)).astype(f32)
    v[..., 3] = 1.0
    return v.astype(np.float16).view(np.uint16)
