"""numpy restatement of sah_sharpen (include/sah_sharpen.h): the ABI-defined arithmetic, operator by operator in fp32.  min and max are the
selects of the header (a < b ? a : b, a > b ? a : b), so a NaN operand behaves as it does there."""
import numpy as np

f32 = np.float32
TILE = (64, 16)  # the kernel's tile (sharpen.hip): four adjacent pixels of a row per thread
DENOISE = 1
DEFAULTS = dict(sharpness=1.0, pre_scale=1.0, flags=0)
K_MIN, K_MAX = f32(2.0 ** -20), f32(2.0 ** 20)
LOBE_LIMIT = f32(-0.1875)
M_LIMIT = f32(1.0) - f32(2.0 ** -17)
HALF_MAX = f32(65504.0)


def settings_of(settings=None):
    s = dict(DEFAULTS)
    s.update(settings or {})
    return s


def fmin(a, b):
    return np.where(a < b, a, b)


def fmax(a, b):
    return np.where(a > b, a, b)


def scale_of(pre_scale, exposure=None):
    """k: pre_scale, or pre_scale * exposure where that is finite and within [2^-20, 2^20].  exposure: a float (the device state's first
    word) or None"""
    k = f32(pre_scale)
    if exposure is None:
        return k
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        kp = k * f32(exposure)
    return kp if (np.isfinite(kp) and kp >= K_MIN and kp <= K_MAX) else k


def clean(scene):
    """(H, W) bool: the three colour channels are finite and none is < 0 (-0 is clean)"""
    c = scene.view(np.float16)[..., :3].astype(f32)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(c) & ~(c < 0)).all(-1)


def _shifted(a, dy, dx):
    """a[y + dy, x + dx] with the coordinates clamped to the image"""
    h, w = a.shape[:2]
    return a[np.clip(np.arange(h) + dy, 0, h - 1)][:, np.clip(np.arange(w) + dx, 0, w - 1)]


def eligible(scene):
    ok = clean(scene)
    return ok & _shifted(ok, -1, 0) & _shifted(ok, 0, -1) & _shifted(ok, 0, 1) & _shifted(ok, 1, 0)


def compress(scene, k):
    """(H, W, 3) float32: every texel on its own, c' = c * k, t = c' / (1 + max(c'))"""
    c = scene.view(np.float16)[..., :3].astype(f32) * f32(k)
    m = fmax(fmax(c[..., 0], c[..., 1]), c[..., 2])
    return c / (f32(1.0) + m)[..., None]


def luma(t):
    return (t[..., 0] * f32(0.5) + t[..., 1]) + t[..., 2] * f32(0.5)


def resolve(t, sharpness, flags):
    """the compressed image t (H, W, 3) -> (s (H, W, 3) in [0, 1], lobe (H, W))"""
    b, d, e, f, h = _shifted(t, -1, 0), _shifted(t, 0, -1), t, _shifted(t, 0, 1), _shifted(t, 1, 0)
    mn4 = fmin(fmin(fmin(b, d), f), h)
    mx4 = fmax(fmax(fmax(b, d), f), h)
    hit_min = np.where(mx4 > 0, fmin(mn4, e) / (f32(4.0) * mx4), f32(0.0))
    hit_max = (f32(1.0) - fmax(mx4, e)) / (f32(4.0) * mn4 - f32(4.0))
    lobe_c = fmax(-hit_min, hit_max)
    lobe = fmax(LOBE_LIMIT, fmin(fmax(fmax(lobe_c[..., 0], lobe_c[..., 1]), lobe_c[..., 2]), f32(0.0))) * f32(sharpness)
    if flags & DENOISE:
        lb, ld, le, lf, lh = luma(b), luma(d), luma(e), luma(f), luma(h)
        nz = ((lb + ld) + (lf + lh)) * f32(0.25) - le
        rng = fmax(fmax(fmax(fmax(lb, ld), le), lf), lh) - fmin(fmin(fmin(fmin(lb, ld), le), lf), lh)
        q = np.where(rng > 0, fmin(np.abs(nz) / rng, f32(1.0)), f32(0.0))
        lobe = lobe * (f32(1.0) - q * f32(0.5))
    lobe3 = lobe[..., None]
    s = (lobe3 * ((b + d) + (f + h)) + e) / (f32(4.0) * lobe3 + f32(1.0))
    return fmin(fmax(s, f32(0.0)), f32(1.0)), lobe


def expand(s, k):
    m = fmin(fmax(fmax(s[..., 0], s[..., 1]), s[..., 2]), M_LIMIT)
    return fmin((s / (f32(1.0) - m)[..., None]) / f32(k), HALF_MAX)


def sharpen(scene, exposure=None, settings=None, rows=(0, 0), out=None, details=False):
    """sah_sharpen.  scene (H, W, 4) uint16 (half bits); exposure: the float of the device state, or None for a NULL state; rows [begin, end)
    of `out` (default: a plane of 0xA5A5), (0, 0) = all rows.  Returns the new `out`; with details also the fp32 o, the compressed s and
    the eligibility mask of the whole image."""
    s_ = settings_of(settings)
    h = scene.shape[0]
    r0, r1 = (0, h) if tuple(rows) == (0, 0) else rows
    out = np.full(scene.shape, 0xA5A5, np.uint16) if out is None else out.copy()
    k = scale_of(s_["pre_scale"], exposure)
    with np.errstate(all="ignore"):
        s, _ = resolve(compress(scene, k), s_["sharpness"], s_["flags"])
        o = expand(s, k)
        halfs = o.astype(np.float16).view(np.uint16)
    ok = eligible(scene)
    full = scene.copy()
    full[..., :3] = np.where(ok[..., None], halfs, scene[..., :3])
    out[r0:r1] = full[r0:r1]
    return (out, o, s, ok) if details else out


def blocky_inputs(w, h, seed, unclean=0):
    """The GPU tests' main input: 3 x 4-texel blocks of values in [0.1, 0.9] times 1 + 0.02 noise, a random alpha; `unclean` texels of
    NaN, +inf, -1 (and -0, which is clean) planted at random places."""
    g = np.random.default_rng(seed)
    blocks = g.uniform(0.1, 0.9, ((h + 3) // 4, (w + 2) // 3, 3))
    img = np.repeat(np.repeat(blocks, 4, 0), 3, 1)[:h, :w] * (1.0 + 0.02 * g.standard_normal((h, w, 3)))
    scene = np.concatenate([img, g.uniform(0, 1, (h, w, 1))], -1).astype(np.float16)
    kinds = [(np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -1.0), (-0.0, 0.25, 0.5), (-np.inf, np.nan, 0.0)]
    flat = scene.reshape(-1, 4)
    for i, at in enumerate(g.choice(w * h, min(unclean, w * h), replace=False)):
        flat[at, :3] = kinds[i % len(kinds)]
    return scene.view(np.uint16)
