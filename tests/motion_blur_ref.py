"""numpy restatement of sah_motion_blur (include/sah_motion_blur.h), operator by operator and bit for bit: fp32 throughout, every operator
rounded on its own, IEEE division and square root, clamp01 and the comparisons as the header spells them.  Every tap of every pixel is
evaluated.  Also the inputs the tests, the fixture and the GPU parity share: an analytic near box in front of a far wall, and the vectors
of a pan and of a dolly formed analytically.

Planes are numpy arrays of bit patterns: scene and out (H, W, 4) uint16, motion_vectors and tiles (h, w, 2) uint16, depth (h, w) float32."""
import numpy as np

f32 = np.float32
DITHER = 1
TILE = 16
FAR = f32(2.0 ** 100)
INF = f32(np.inf)
BAYER = np.array([0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5], np.int64)
DEFAULTS = dict(shutter=0.5, max_blur_pixels=32.0, min_velocity_pixels=0.5, sample_count=12, depth_extent=1.0, z_near=0.1, jitter=(0.0, 0.0),
                previous_jitter=(0.0, 0.0), flags=0)


def h2f(bits):
    return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16).astype(f32)


def f2h(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, f32).astype(np.float16).view(np.uint16)


def to_half_bits(x):
    """float array -> the uint16 patterns of its halfs (round to nearest even)"""
    return f2h(np.asarray(x, f32))


def clamp01(a):
    return np.where(a > 0, np.where(a < 1, a, f32(1)), f32(0)).astype(f32)


def floor_to_int(v):
    return np.minimum(np.maximum(np.floor(v), f32(-2147483648.0)), f32(2147483520.0)).astype(np.int64)


def pair_bits(mv):
    """(.., 2) uint16 -> uint32 x | y << 16"""
    mv = np.asarray(mv, np.uint16)
    return mv[..., 0].astype(np.uint32) | (mv[..., 1].astype(np.uint32) << np.uint32(16))


def bits_pair(m):
    m = np.asarray(m, np.uint32)
    return np.stack([(m & np.uint32(0xFFFF)).astype(np.uint16), (m >> np.uint32(16)).astype(np.uint16)], -1)


class Params:
    def __init__(self, **changes):
        unknown = set(changes) - set(DEFAULTS)
        assert not unknown, unknown
        v = dict(DEFAULTS)
        v.update(changes)
        self.shutter, self.max_blur, self.min_velocity = f32(v["shutter"]), f32(v["max_blur_pixels"]), f32(v["min_velocity_pixels"])
        self.n, self.extent, self.z_near, self.flags = int(v["sample_count"]), f32(v["depth_extent"]), f32(v["z_near"]), int(v["flags"])
        self.jx, self.jy = f32(v["jitter"][0]), f32(v["jitter"][1])
        self.djx, self.djy = f32(v["previous_jitter"][0]) - self.jx, f32(v["previous_jitter"][1]) - self.jy


def scaled(m, p):
    """Velocity up to the clamp: (a.x, a.y, l2) of pairs m (uint32), zero where l2 is not finite"""
    with np.errstate(all="ignore"):
        ax = ((h2f(m & np.uint32(0xFFFF)) + p.djx) * p.shutter).astype(f32)
        ay = ((h2f(m >> np.uint32(16)) + p.djy) * p.shutter).astype(f32)
        l2 = (ax * ax + ay * ay).astype(f32)
    bad = ~(l2 < INF)
    zero = f32(0)
    return np.where(bad, zero, ax), np.where(bad, zero, ay), np.where(bad, zero, l2)


def velocity(m, p):
    """Velocity: (v.x, v.y, |v|) of pairs m"""
    ax, ay, l2 = scaled(m, p)
    l = np.sqrt(l2).astype(f32)
    over = l > p.max_blur
    with np.errstate(all="ignore"):
        s = (p.max_blur / l).astype(f32)
        return (np.where(over, ax * s, ax).astype(f32), np.where(over, ay * s, ay).astype(f32), np.where(over, p.max_blur, l).astype(f32))


def key(m, p):
    """Key: (l2, bit pattern) as one uint64"""
    m = np.asarray(m, np.uint32)
    l2 = np.ascontiguousarray(scaled(m, p)[2], dtype=f32)
    return (l2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | m.astype(np.uint64)


def tile_vectors(mv, p):
    """Tile: (ceil(h / 16), ceil(w / 16), 2) uint16, the raw pair with the greatest key per tile"""
    m = pair_bits(mv)
    h, w = m.shape
    th, tw = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    k = np.zeros((th * TILE, tw * TILE), np.uint64)  # 0: outside the image, below key + 1 of any texel
    k[:h, :w] = key(m, p) + np.uint64(1)
    best = k.reshape(th, TILE, tw, TILE).max(axis=(1, 3)) - np.uint64(1)
    return bits_pair((best & np.uint64(0xFFFFFFFF)).astype(np.uint32))


def neighbour_vectors(tiles, p, reach=1):
    """Neighbour: per tile, the pair with the greatest key among the (2 reach + 1)^2 tiles around it, clamped to the grid"""
    k = key(pair_bits(tiles), p)
    th, tw = k.shape
    padded = np.pad(k, reach, mode="edge") if reach else k
    best = k.copy()
    for dy in range(2 * reach + 1):
        for dx in range(2 * reach + 1):
            best = np.maximum(best, padded[dy:dy + th, dx:dx + tw])
    return (best & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def surface(d, p):
    with np.errstate(all="ignore"):
        z = np.where(d > 0, (p.z_near / d).astype(f32), FAR).astype(f32)
    return np.where(z < FAR, z, FAR).astype(f32)


def clean(rgb):
    return ((rgb >= 0) & (rgb < INF)).all(-1)


def sample_positions(n_out, n_render, jitter):
    s = f32(n_render) / f32(n_out)
    u = ((np.arange(n_out).astype(f32) + f32(0.5)) * s).astype(f32) - f32(jitter)
    return u.astype(f32), np.clip(floor_to_int(u), 0, n_render - 1)


def _cone(d, s):
    return clamp01(f32(1) - (d / s).astype(f32))


def _cyl(d, s):
    e0, e1 = (f32(0.95) * s).astype(f32), (f32(1.05) * s).astype(f32)
    y = clamp01(((e1 - d) / (e1 - e0)).astype(f32))
    return ((y * y) * (f32(3) - f32(2) * y)).astype(f32)


def motion_blur_ex(scene, depth, mv, reach=1, **params):
    """-> (out, info): out (H, W, 4) uint16; info["passed"] (H, W) bool, whether the pixel passed through; info["sw"] (H, W) float32, its
    sum of weights (0 where the taps were never run); info["tiles"] the tile plane; info["speed"] (H, W) the neighbour speed |vn|.
    reach = 1 is the contract's 3 x 3 tile neighbourhood (0: the pixel's own tile alone, for the test that shows why that is not enough)."""
    p = Params(**params)
    scene = np.ascontiguousarray(scene).view(np.uint16)
    mv = np.ascontiguousarray(mv).view(np.uint16)
    depth = np.asarray(depth, f32)
    H, W = scene.shape[:2]
    h, w = depth.shape
    assert mv.shape == (h, w, 2) and w <= W and h <= H and p.n % 2 == 0 and 2 <= p.n <= 32
    rx, ry = f32(W) / f32(w), f32(H) / f32(h)
    tiles = tile_vectors(mv, p)
    nb = neighbour_vectors(tiles, p, reach)
    ux1, i1 = sample_positions(W, w, p.jx)
    uy1, j1 = sample_positions(H, h, p.jy)
    ux, uy = np.broadcast_to(ux1[None, :], (H, W)), np.broadcast_to(uy1[:, None], (H, W))
    i, j = np.broadcast_to(i1[None, :], (H, W)), np.broadcast_to(j1[:, None], (H, W))
    vnx, vny, vn = velocity(nb[j >> 4, i >> 4], p)
    m = pair_bits(mv)
    _, _, vp = velocity(m[j, i], p)
    zp = surface(depth[j, i], p)
    c = h2f(scene[..., :3])
    moving = ~(vn < p.min_velocity)
    run = moving & clean(c)
    Y, X = np.mgrid[0:H, 0:W]
    dith = ((BAYER[(X & 3) + 4 * (Y & 3)].astype(f32) - f32(7.5)) * f32(0.0625)).astype(f32) if p.flags & DITHER else np.zeros((H, W), f32)
    nf, half = f32(p.n), f32(0.5)
    sw, acc = np.zeros((H, W), f32), np.zeros((H, W, 3), f32)
    with np.errstate(all="ignore"):
        for k in range(p.n):
            t = (((f32(k) + half) + dith) / nf).astype(f32) - half
            ex, ey = (vnx * t).astype(f32), (vny * t).astype(f32)
            px, py = (ux + ex).astype(f32), (uy + ey).astype(f32)
            ok = run & (px >= 0) & (px < f32(w)) & (py >= 0) & (py < f32(h))
            qx, qy = (px * rx).astype(f32), (py * ry).astype(f32)
            ok &= (qx >= 0) & (qx < f32(W)) & (qy >= 0) & (qy < f32(H))
            safe = lambda v, n: np.clip(np.where(ok, np.floor(np.where(ok, v, 0)), 0).astype(np.int64), 0, n - 1)  # noqa: E731
            ti, tj, si, sj = safe(px, w), safe(py, h), safe(qx, W), safe(qy, H)
            s = h2f(scene[sj, si, :3])
            ok &= clean(s)
            _, _, vs = velocity(m[tj, ti], p)
            zs = surface(depth[tj, ti], p)
            d = np.sqrt((ex * ex + ey * ey).astype(f32)).astype(f32)
            f = clamp01(f32(1) - ((zs - zp) / p.extent).astype(f32))
            g = clamp01(f32(1) - ((zp - zs) / p.extent).astype(f32))
            wk = ((f * _cone(d, vs) + g * _cone(d, vp)).astype(f32) + (f32(2) * _cyl(d, vs)) * _cyl(d, vp)).astype(f32)
            use = ok & (wk != 0)
            sw = np.where(use, sw + wk, sw).astype(f32)
            acc = np.where(use[..., None], acc + wk[..., None] * (s - c), acc).astype(f32)
        r = (acc / sw[..., None]).astype(f32)
        o = (c + r).astype(f32)
        blurred = run & (sw != 0) & (np.abs(o) < INF).all(-1)
    out = scene.copy()
    out[..., :3] = np.where(blurred[..., None] & (r != 0), f2h(o), scene[..., :3])
    return out, dict(passed=~blurred, sw=sw, tiles=tiles, speed=vn, moving=moving)


def motion_blur(scene, depth, mv, **params):
    return motion_blur_ex(scene, depth, mv, **params)[0]


# ---- the inputs the tests share ----------------------------------------------------------------------------------------------------------------
Z_NEAR, Z_BOX, Z_WALL = f32(0.1), f32(2.0), f32(10.0)


def box_mask(w, h, box=(0.3, 0.25, 0.6, 0.75)):
    """the near box: a rectangle given in fractions of the frame"""
    y, x = np.mgrid[0:h, 0:w]
    return (x >= int(box[0] * w)) & (x < int(box[2] * w)) & (y >= int(box[1] * h)) & (y < int(box[3] * h))


def box_depth(w, h, box=(0.3, 0.25, 0.6, 0.75)):
    """reversed-Z depth of the box (z = 2) in front of the wall (z = 10), z_near 0.1"""
    z = np.where(box_mask(w, h, box), Z_BOX, Z_WALL).astype(f32)
    return (Z_NEAR / z).astype(f32)


def textured_scene(W, H, seed):
    """an HDR image with detail at every scale, so that any blur moves bits: halfs in [0, 4), alpha a ramp"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.5 * np.sin(x[..., None] * np.array([0.9, 0.37, 0.11]) + y[..., None] * np.array([0.23, 0.71, 0.05]))
    rgb = base * 2.0 + g.random((H, W, 3)) * 2.0
    alpha = (x + y) / float(W + H)
    return to_half_bits(np.concatenate([rgb, alpha[..., None]], -1))


def pan_vectors(w, h, vector):
    """a pan: every texel moved by the same vector (previous position - pixel centre), in render pixels"""
    return to_half_bits(np.broadcast_to(np.asarray(vector, f32), (h, w, 2)))


def dolly_vectors(w, h, depth, advance, z_near=Z_NEAR):
    """a dolly of `advance` view-space units towards the scene: a point at linear depth z was at distance z + advance one frame ago, so its
    previous position is centre + (p - centre) * z / (z + advance)"""
    y, x = np.mgrid[0:h, 0:w]
    z = (f32(z_near) / depth).astype(np.float64)
    scale = z / (z + advance) - 1.0
    return to_half_bits(np.stack([(x + 0.5 - 0.5 * w) * scale, (y + 0.5 - 0.5 * h) * scale], -1))


def static_vectors(w, h, jitter, previous_jitter):
    """what sah_motion_vectors_render writes under a static camera: jitter - previous_jitter, as halfs"""
    d = np.asarray(jitter, f32) - np.asarray(previous_jitter, f32)
    return to_half_bits(np.broadcast_to(d, (h, w, 2)))
