"""numpy restatement of sah_ssr (include/sah_ssr.h): the plain march, step for step and bit for bit — fp32 operators throughout, every one
rounded on its own, IEEE division and square root, clamps and min / max as the comparisons the header spells out.  Every sample of every
ray is evaluated.  Also the inputs the tests share: random G-buffers, the analytic mirror room,
and the list of cases the GPU parity runs over (tests/test_ssr_cpu.py asserts that the list exercises every outcome)."""
import numpy as np

from tests.ssao_ref import View, linear_depth, positions, random_inputs

f32 = np.float32
JITTER, REFLECTION_ONLY = 1, 2
BLOCK = 8            # the scratch plane's block (include/sah_ssr.h), for the extents the tests choose
TRACE_TILE = (32, 8)  # k_ssr_trace's workgroup tile: four waves of 8 x 8 pixels side by side
BAYER = np.array([0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5], np.int64)
DEFAULTS = dict(max_distance=50.0, thickness=0.5, stride_pixels=4.0, max_steps=64, refine_steps=4, max_roughness=0.6, edge_fade=0.1,
                intensity=1.0, flags=0)
# pass-through reasons and ray outcomes of info["outcome"]
NO_SURFACE, NOT_FINITE, ROUGH, NO_INTENSITY, MISS_RAY, MISS_T, MISS_IMAGE, MISS_STEPS, REJECTED, HIT = range(10)
OUTCOMES = {NO_SURFACE: "pass-through: no surface", NOT_FINITE: "pass-through: P or N not finite", ROUGH: "pass-through: rough",
            NO_INTENSITY: "pass-through: intensity 0", MISS_RAY: "miss: degenerate ray", MISS_T: "miss: t > 1", MISS_IMAGE: "miss: left the image",
            MISS_STEPS: "miss: max_steps", REJECTED: "rejected hit", HIT: "hit"}


def srgb_lut():
    """sRGB8 -> linear, the Vulkan EOTF in double rounded to fp32 (the library's table, api.cpp: sah_create)"""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(f32)


def unorm_lut():
    return (np.arange(256, dtype=f32) / f32(255.0)).astype(f32)


def clamp01(x):
    return np.where(x > 0, np.where(x < 1, x, f32(1)), f32(0)).astype(f32)


def fmin(a, b):
    return np.where(a < b, a, b).astype(f32)


def view_normals(normals, view):
    """Centre of sah_ssao.h: the unit view-space normal of every texel"""
    n = np.ascontiguousarray(normals).view(np.float16)[..., :3].astype(f32)
    m = view.view
    nv = np.stack([(m[0] * n[..., 0] + m[4] * n[..., 1]) + m[8] * n[..., 2],
                   (m[1] * n[..., 0] + m[5] * n[..., 1]) + m[9] * n[..., 2],
                   (m[2] * n[..., 0] + m[6] * n[..., 1]) + m[10] * n[..., 2]], -1).astype(f32)
    nl = np.sqrt((nv[..., 0] * nv[..., 0] + nv[..., 1] * nv[..., 1]) + nv[..., 2] * nv[..., 2])
    return (nv / nl[..., None]).astype(f32)


def project(Q, zq, p_axis, p2, half):
    return ((((Q * p_axis) / zq) - p2) + f32(1)) * half


class Rays:
    """what step "Ray" of the header forms for every pixel, and sample(t) / sample_index(i)"""

    def __init__(self, P, z, N, view, w, h, p):
        self.w, self.h = w, h
        hw, hh = f32(0.5) * f32(w), f32(0.5) * f32(h)
        pl = np.sqrt((P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2])
        V = (P / pl[..., None]).astype(f32)
        self.nv = (N[..., 0] * V[..., 0] + N[..., 1] * V[..., 1]) + N[..., 2] * V[..., 2]
        nv2 = f32(2) * self.nv
        self.R = R = (V - nv2[..., None] * N).astype(f32)
        length = np.full(z.shape, f32(p["max_distance"]), f32)
        lim = (z - view.z_near) / R[..., 2]
        length = np.where((R[..., 2] > 0) & (lim < length), lim, length).astype(f32)
        E = (P + R * length[..., None]).astype(f32)
        ze = -E[..., 2]
        ze = np.where(ze > view.z_near, ze, view.z_near).astype(f32)
        self.s0x, self.s0y = project(P[..., 0], z, view.p00, view.p20, hw), project(P[..., 1], z, view.p11, view.p21, hh)
        s1x, s1y = project(E[..., 0], ze, view.p00, view.p20, hw), project(E[..., 1], ze, view.p11, view.p21, hh)
        self.k0 = f32(1) / z
        k1 = f32(1) / ze
        self.dsx, self.dsy, self.dk = s1x - self.s0x, s1y - self.s0y, k1 - self.k0
        ax, ay = np.abs(self.dsx), np.abs(self.dsy)
        self.L = np.where(ax > ay, ax, ay).astype(f32)
        self.ok = (ax < np.inf) & (ay < np.inf) & (self.L >= 1) & (self.k0 < np.inf)
        ys, xs = np.mgrid[0:h, 0:w]
        self.jit = (BAYER[(xs & 3) + 4 * (ys & 3)].astype(f32) * f32(0.0625)) if int(p["flags"]) & JITTER else np.zeros((h, w), f32)
        self.stride = f32(p["stride_pixels"])

    def t_of(self, i):
        return (((f32(i) + self.jit) * self.stride) / self.L).astype(f32)

    def sample(self, t):
        """-> (inside, ix, iy, zr) of the sample at parameter t (ix, iy are 0 where it lies outside)"""
        sx, sy = self.s0x + t * self.dsx, self.s0y + t * self.dsy
        k = self.k0 + t * self.dk
        zr = (f32(1) / k).astype(f32)
        inside = (sx >= 0) & (sx < f32(self.w)) & (sy >= 0) & (sy < f32(self.h))
        ix, iy = np.where(inside, np.floor(sx), 0).astype(np.int64), np.where(inside, np.floor(sy), 0).astype(np.int64)
        return inside, ix, iy, zr


def ssr_ex(color, normals, data, depth, source, lit, view, params=None, rows=None, out=None):
    """color, data (H, W, 4) uint8; normals, source, lit (H, W, 4) uint16; depth (H, W) float32; view a ssao_ref.View.
    -> (out (H, W, 4) uint16, info).  Rows outside `rows` hold what `out` held (zeros without one)."""
    p = dict(DEFAULTS, **(params or {}))
    depth = np.ascontiguousarray(depth, f32)
    h, w = depth.shape
    rows = (0, h) if rows is None or tuple(rows) == (0, 0) else tuple(rows)
    flags = int(p["flags"])
    thickness, max_rough, intensity = f32(p["thickness"]), f32(p["max_roughness"]), f32(p["intensity"])
    lit = np.ascontiguousarray(lit).view(np.uint16).reshape(h, w, 4)
    source = np.ascontiguousarray(source).view(np.uint16).reshape(h, w, 4)
    with np.errstate(all="ignore"):
        surface, z = linear_depth(depth, view.z_near)
        P = positions(z, view, w, h)
        N = view_normals(normals, view)
        s_lut, u_lut = srgb_lut(), unorm_lut()
        rough, metal = u_lut[data[..., 1]], u_lut[data[..., 2]]
        base = s_lut[color[..., :3]]
        f0 = (f32(0.04) + (base - f32(0.04)) * metal[..., None]).astype(f32)
        outcome = np.full((h, w), -1, np.int64)
        outcome[~surface] = NO_SURFACE
        outcome[(outcome < 0) & ~(np.isfinite(P).all(-1) & np.isfinite(N).all(-1))] = NOT_FINITE
        outcome[(outcome < 0) & ~(rough < max_rough)] = ROUGH
        if intensity == 0:
            outcome[outcome < 0] = NO_INTENSITY
        rays = Rays(P, z, N, view, w, h, p)
        outcome[(outcome < 0) & ~rays.ok] = MISS_RAY
        active = outcome < 0
        hit_i = np.zeros((h, w), np.int64)
        behind = np.zeros((h, w), np.int64)
        zr_first = {}
        for i in range(1, int(p["max_steps"]) + 1):
            if not active.any():
                break
            t = rays.t_of(i)
            ended = active & (t > 1)
            outcome[ended] = MISS_T
            active &= ~ended
            inside, ix, iy, zr = rays.sample(t)
            left = active & ~inside
            outcome[left] = MISS_IMAGE
            active &= ~left
            has = surface[iy, ix]
            dz = zr - z[iy, ix]
            hit = active & has & (dz >= 0) & (dz <= thickness)
            behind += active & has & (dz > thickness)
            hit_i[hit] = i
            outcome[hit] = HIT
            active &= ~hit
        outcome[active] = MISS_STEPS
        # refinement
        found = outcome == HIT
        lo, hi = rays.t_of(np.maximum(hit_i - 1, 0).astype(f32)), rays.t_of(hit_i.astype(f32))
        moved = np.zeros((h, w), bool)
        for _ in range(int(p["refine_steps"])):
            mid = ((lo + hi) * f32(0.5)).astype(f32)
            inside, ix, iy, zr = rays.sample(mid)
            passes = inside & surface[iy, ix] & (zr >= z[iy, ix])
            moved |= found & passes
            hi, lo = np.where(passes, mid, hi).astype(f32), np.where(passes, lo, mid).astype(f32)
        inside, hx, hy, _ = rays.sample(hi)
        hx, hy = np.where(found, hx, 0), np.where(found, hy, 0)
        src = source[hy, hx].view(np.float16)[..., :3].astype(f32)
        clean = ((src >= 0) & (src < np.inf)).all(-1)
        Nh, R = N[hy, hx], rays.R
        facing = ((Nh[..., 0] * R[..., 0] + Nh[..., 1] * R[..., 1]) + Nh[..., 2] * R[..., 2]) < 0
        outcome[found & ~(clean & facing)] = REJECTED
        found = outcome == HIT
        # weight and result
        m = f32(1) - clamp01(-rays.nv)
        m2 = m * m
        m5 = (m2 * m2) * m
        F = (f0 + (f32(1) - f0) * m5[..., None]).astype(f32)
        rf = clamp01(f32(1) - rough / max_rough)
        u, v = (hx.astype(f32) + f32(0.5)) / f32(w), (hy.astype(f32) + f32(0.5)) / f32(h)
        e = fmin(fmin(u, f32(1) - u), fmin(v, f32(1) - v))
        ef = clamp01(e / f32(p["edge_fade"]))
        tf = clamp01(f32(1) - hi)
        wgt = (((intensity * rf) * ef) * tf).astype(f32)
        g = (wgt[..., None] * F).astype(f32)
        litf = lit.view(np.float16)[..., :3].astype(f32)
        if flags & REFLECTION_ONLY:
            res = np.zeros((h, w, 4), np.float16)
            res[..., :3] = (g * src).astype(np.float16)
            res[..., 3] = wgt.astype(np.float16)
            res = np.where(found[..., None], res.view(np.uint16), np.uint16(0))
        else:
            res = lit.copy()
            res[..., :3] = np.where(found[..., None], (litf + g * src).astype(np.float16).view(np.uint16), lit[..., :3])
    result = np.zeros((h, w, 4), np.uint16) if out is None else np.array(out, np.uint16).reshape(h, w, 4)
    result[rows[0]:rows[1]] = res[rows[0]:rows[1]]
    info = dict(outcome=outcome, behind=behind, hit_index=hit_i, refined=found & moved, hit=found, hx=hx, hy=hy, t_hit=hi, weight=wgt, rays=rays,
                surface=surface, z=z)
    return result, info


def ssr(*args, **kwargs):
    return ssr_ex(*args, **kwargs)[0]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def halfs(a):
    return np.ascontiguousarray(np.asarray(a, np.float16)).view(np.uint16)


def random_frame(w, h, seed):
    """dict of the seven input planes: ssao_ref.random_inputs plus random colour, data (a third of the pixels smooth) and HDR source / lit"""
    g = np.random.default_rng(seed + 5000)
    depth, normals = random_inputs(w, h, seed)
    color = g.integers(0, 256, (h, w, 4), dtype=np.uint8)
    data = g.integers(0, 256, (h, w, 4), dtype=np.uint8)
    data[..., 1] = np.where(g.random((h, w)) < 0.7, g.integers(0, 120, (h, w)), data[..., 1])  # mostly below the default max_roughness
    source = halfs(g.uniform(0, 4, (h, w, 4)) ** 2)
    lit = halfs(g.uniform(0, 2, (h, w, 4)))
    if w * h >= 12:
        cells = g.permutation(w * h)[:max(3, w * h // 16)]
        kinds = g.integers(0, 3, cells.size)
        flat = source.reshape(-1, 4)
        flat[cells[kinds == 0], 0] = 0x7e00  # NaN
        flat[cells[kinds == 1], 1] = 0x7c00  # +inf
        flat[cells[kinds == 2], 2] = 0xbc00  # -1
    return dict(color=color, normals=normals, data=data, depth=depth, source=source, lit=lit)


ROOM_VIEW = dict(p00=1.0, p11=16.0 / 9.0, p20=0.002, p21=-0.003, z_near=0.05)
ROOM = dict(floor_y=1.0, wall_z=10.0, wall_top=-3.0)  # view space, y down as the image's rows run: floor below the eye, sky above the wall


def room_view():
    return View.of(**ROOM_VIEW)


def mirror_room(w, h, seed=0, rough_code=20):
    """A floor plane, a striped back wall and sky above it, built analytically in view space (identity view matrix; y grows down the image).
    The floor is metal of roughness rough_code / 255; the wall is rough.  source: stripes of one colour per row on the wall, random on the floor."""
    g = np.random.default_rng(seed + 9000)
    v = room_view()
    tx, ty = f32(2) / f32(w), f32(2) / f32(h)
    ndx = (np.arange(w, dtype=np.float64)[None, :] + 0.5) * float(tx) - 1 + float(v.p20)
    ndy = (np.arange(h, dtype=np.float64)[:, None] + 0.5) * float(ty) - 1 + float(v.p21)
    dy = np.broadcast_to(ndy / float(v.p11), (h, w))  # view-space y per unit of linear depth
    with np.errstate(all="ignore"):
        z_floor = np.where(dy > 0, ROOM["floor_y"] / dy, np.inf)
    floor = z_floor < ROOM["wall_z"]
    wall = ~floor & (ROOM["wall_z"] * dy >= ROOM["wall_top"])
    z = np.where(floor, z_floor, ROOM["wall_z"])
    depth = np.where(floor | wall, float(v.z_near) / z, 0.0).astype(f32)
    normals = np.zeros((h, w, 4), np.float16)
    normals[floor, 1] = -1.0
    normals[wall, 2] = 1.0
    data = np.zeros((h, w, 4), np.uint8)
    data[..., 1] = np.where(floor, rough_code, 230)
    data[..., 2] = np.where(floor, 255, 0)
    color = np.full((h, w, 4), 200, np.uint8)
    stripes = np.stack([(np.arange(h) % 5 + 1) * 0.5, (np.arange(h) % 3 + 1) * 0.25, np.arange(h) * 0.125 + 0.125, np.ones(h)], -1)
    source = np.where(wall[..., None], stripes[:, None, :], g.uniform(0, 1, (h, w, 4)))
    lit = g.uniform(0, 1, (h, w, 4))
    _ = ndx
    return dict(color=color, normals=normals.view(np.uint16), data=data, depth=depth, source=halfs(source), lit=halfs(lit)), dict(floor=floor, wall=wall)


def transposed_room(w, h, seed=0):
    """the mirror room of h x w turned about the image's diagonal into a w x h frame: the floor lies to the right, the wall's stripes run
    down the columns and the rays run along the rows.  -> (frame, masks, View)"""
    frame, masks = mirror_room(h, w, seed)
    turned = {k: np.ascontiguousarray(np.swapaxes(v, 0, 1)) for k, v in frame.items()}
    n = turned["normals"].copy()
    n[..., 0], n[..., 1] = turned["normals"][..., 1], turned["normals"][..., 0]
    turned["normals"] = n
    v = ROOM_VIEW
    return turned, {k: m.T for k, m in masks.items()}, View.of(v["p11"], v["p00"], v["p21"], v["p20"], v["z_near"])


def mirror_row(y, h):
    """the image row at which the mirror ray of a floor pixel of row y meets the wall, from the room's geometry in fp64"""
    v = ROOM_VIEW
    dy = ((y + 0.5) * 2.0 / h - 1 + v["p21"]) / v["p11"]
    zf = ROOM["floor_y"] / dy                               # the floor point (.., floor_y, -zf); the mirrored ray keeps x / z and flips y
    y_wall = ROOM["floor_y"] - dy * (ROOM["wall_z"] - zf)   # y of the ray at the wall
    return ((y_wall / ROOM["wall_z"]) * v["p11"] - v["p21"] + 1) * 0.5 * h


EXTENTS = [(1, 1), (2, 3), (7, 9), (8, 8), (9, 7), (15, 17), (64, 16), (65, 17), (192, 48), (31, 7), (32, 8), (33, 9)]
RANDOM_SETTINGS = [dict(stride_pixels=1.0, max_steps=256, refine_steps=0, thickness=0.0, flags=0),
                   dict(stride_pixels=2.5, max_steps=7, refine_steps=4, thickness=0.5, flags=JITTER),
                   dict(stride_pixels=4.0, max_steps=1, refine_steps=8, thickness=3e38, flags=REFLECTION_ONLY),
                   dict(stride_pixels=1.0, max_steps=256, refine_steps=8, thickness=0.5, flags=JITTER | REFLECTION_ONLY),
                   dict(stride_pixels=4.0, max_steps=7, refine_steps=4, thickness=3e38, flags=0),
                   dict(stride_pixels=2.5, max_steps=256, refine_steps=4, thickness=0.5, flags=0, max_distance=4.0)]
ROOM_SETTINGS = dict(thickness=4.0, stride_pixels=2.0, max_steps=128, max_distance=20.0)
FAR_SETTINGS = dict(max_distance=1.0e6, stride_pixels=4.0, max_steps=256)  # at 192 x 48: most rays leave the image


def far_frame(w, h, seed):
    """random_frame with its bumps smoothed away — a tilted plane four to ten units off, the planted sky, NaN, negative and infinite depths
    kept — under the same random normals: little stands in a ray's way, so with a long max_distance most rays run off the image"""
    frame = random_frame(w, h, seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = frame["depth"]
    ordinary = np.isfinite(d) & (d > 0)
    frame["depth"] = np.where(ordinary, (0.05 / (4.0 + 0.02 * xx + 0.03 * yy)).astype(f32), d).astype(f32)
    return frame


def random_view(w, h):
    """the projection of a 75-degree camera of aspect w / h with a sub-pixel jitter, and a turned view matrix"""
    c, s = np.cos(0.4), np.sin(0.4)
    f = 1.0 / np.tan(np.radians(75.0) / 2)
    return View.of(f * h / w if w >= h else f, f if w >= h else f * w / h, 0.3 / w, -0.2 / h, 0.05, [[c, 0, s], [0, 1, 0], [-s, 0, c]])


def parity_cases():
    """(name, frame dict, View, settings) of every comparison tests/test_ssr_gpu.py makes against this restatement over extents"""
    for w, h in EXTENTS:
        frame, view = random_frame(w, h, 11 * w + h), random_view(w, h)
        for n, settings in enumerate(RANDOM_SETTINGS):
            yield f"random {w}x{h} #{n}", frame, view, settings
    for w, h in ((96, 54), (75, 41)):
        yield f"room {w}x{h}", mirror_room(w, h)[0], room_view(), ROOM_SETTINGS
    yield "far 192x48", far_frame(192, 48, 77), random_view(192, 48), FAR_SETTINGS
