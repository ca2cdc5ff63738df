"""numpy restatement of sah_exposure_meter / sah_exposure_apply (include/sah_exposure.h): the ABI-defined arithmetic, operator by operator in
fp32, the histogram and the window in integers.  A state is a 16-byte numpy record (STATE)."""
import numpy as np

f32 = np.float32
BINS = 256
TILE = (128, 4)  # the kernel's tile (exposure.hip): a wave per row of it, two pixels per lane
HISTORY_INVALID = 1
DEFAULTS = dict(key=0.18, low_fraction=0.5, high_fraction=0.95, min_exposure=1.0 / 64.0, max_exposure=64.0, adaptation=1.0, max_workgroups=0, flags=0)
STATE = np.dtype([("exposure", np.float32), ("adapted", np.float32), ("metered", np.uint32), ("window", np.uint32)])
assert STATE.itemsize == 16
QUIET_NAN = np.array([0x7fc00000], np.uint32).view(f32)[0]


def settings_of(settings=None):
    s = dict(DEFAULTS)
    s.update(settings or {})
    return s


def f2u(x):
    """float -> uint32: truncation; a NaN and negatives give 0, 2^32 and more give 2^32 - 1"""
    x = f32(x)
    if not x > 0:
        return 0
    if x >= f32(4294967296.0):
        return 0xffffffff
    return int(x)


def fmin(a, b):
    return a if a < b else b


def fmax(a, b):
    return a if a > b else b


def luminance(scene):
    """scene (H, W, 4) uint16 (half bits).  Returns L (H, W) float32"""
    c = scene.view(np.float16).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (c[..., 0] * f32(0.2126) + c[..., 1] * f32(0.7152)) + c[..., 2] * f32(0.0722)


def bins_of(L):
    """(counted, k): the COUNTED mask and the bin of every pixel (meaningless where not counted)"""
    with np.errstate(invalid="ignore"):
        counted = np.isfinite(L) & (L > 0)
    k = np.clip((L.view(np.uint32) >> 20).astype(np.int64) - 856, 0, 255)
    return counted, k


def histogram(scene):
    counted, k = bins_of(luminance(scene))
    return np.bincount(k[counted].ravel(), minlength=BINS).astype(np.uint32)


def plog(L):
    """the pseudo-log2 of positive floats, in fp64 (for the properties' sake; the ABI never evaluates it)"""
    return np.asarray(L, f32).view(np.uint32).astype(np.float64) / 2.0 ** 23 - 127.0


def window_sum(n, low_fraction, high_fraction):
    """(N, lo, hi, S) of the histogram n"""
    n = [int(v) for v in n]
    N = sum(n[1:])
    assert N < 2 ** 32
    lo = min(f2u(f32(N) * f32(low_fraction)), N)
    hi = min(f2u(f32(N) * f32(high_fraction)), N)
    cl = lambda x: min(max(x, lo), hi)  # noqa: E731
    S, C = 0, 0
    for b in range(1, BINS):
        S += (cl(C + n[b]) - cl(C)) * (2 * b + 1)
        C += n[b]
    return N, lo, hi, S


def l_avg_of(m):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.array([f2u((f32(m) + f32(127.0)) * f32(8388608.0))], np.uint32).view(f32)[0]


def state_from_histogram(n, state_in=None, settings=None):
    s = settings_of(settings)
    N, lo, hi, S = window_sum(n, s["low_fraction"], s["high_fraction"])
    metered = hi > lo
    history = not (s["flags"] & HISTORY_INVALID) and state_in is not None and bool(np.isfinite(state_in["adapted"]))
    if not (s["flags"] & HISTORY_INVALID):
        assert state_in is not None, "state_in may be None only with HISTORY_INVALID"
    out = np.zeros((), STATE)
    out["metered"], out["window"] = N, hi - lo
    lo_e, hi_e, key = f32(s["min_exposure"]), f32(s["max_exposure"]), f32(s["key"])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if metered:
            m_t = (f32(S) / f32(hi - lo)) * f32(0.0625) - f32(20.0)  # (S < 2^53: int -> double is exact, double -> float rounds once)
            m_p = f32(state_in["adapted"]) if history else None
            m = m_p + (m_t - m_p) * f32(s["adaptation"]) if history else m_t
        elif history:
            m = f32(state_in["adapted"])
        else:
            out["exposure"], out["adapted"] = fmin(fmax(f32(1.0), lo_e), hi_e), QUIET_NAN
            return out
        e = key / l_avg_of(m)
    out["exposure"], out["adapted"] = fmin(fmax(e, lo_e), hi_e), m
    return out


def meter(scene, state_in=None, settings=None):
    """sah_exposure_meter without exposed_out: (histogram (256,) uint32, state_out).  state_in: a STATE record or None."""
    n = histogram(scene)
    return n, state_from_histogram(n, state_in, settings)


def apply(scene, exposure, rows=(0, 0), out=None):
    """sah_exposure_apply: rows [begin, end) of `out` (default: a copy of nothing — rows outside the band are 0xA5A5), (0, 0) = all rows"""
    h = scene.shape[0]
    r0, r1 = (0, h) if tuple(rows) == (0, 0) else rows
    out = np.full(scene.shape, 0xA5A5, np.uint16) if out is None else out.copy()
    c = scene[r0:r1].view(np.float16).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        rgb = (c[..., :3] * f32(exposure)).astype(np.float16)
    out[r0:r1, :, :3] = rgb.view(np.uint16)
    out[r0:r1, :, 3] = scene[r0:r1, :, 3]
    return out


def band_rows(rows, h):
    """the rows of `out` a call with `rows` writes"""
    return (0, h) if tuple(rows) == (0, 0) else tuple(rows)


def random_inputs(w, h, seed, median=1.0, sigma=2.5, specials=True):
    """A log-normal scene (sigma in octaves about `median`) with a random alpha, and — with specials, from 64 pixels on — pixels that are
    not counted (zeros, -0, negatives, NaN, +-inf), half denormals, and luminances beyond both ends of the histogram."""
    g = np.random.default_rng(seed)
    lum = median * 2.0 ** g.normal(0.0, sigma, (h, w, 1))
    tint = g.uniform(0.3, 1.7, (h, w, 3))
    with np.errstate(over="ignore"):  # (the tail of a wide image overflows to a half infinity: an uncounted pixel like any other)
        scene = np.concatenate([lum * tint, g.uniform(0, 1, (h, w, 1))], -1).astype(np.float16)
    if specials and w * h >= 64:
        flat = scene.reshape(-1, 4)
        idx = g.choice(w * h, min(w * h // 4, 40), replace=False)
        rows = [(0, 0, 0), (-0.0, -0.0, -0.0), (-1, -2, -3), (np.nan, 1, 1), (np.inf, 1, 1), (-np.inf, 0, 0), (6e-8, 6e-8, 6e-8), (1e-7, 0, 0),
                (65504, 65504, 65504), (3e-7, 3e-7, 3e-7), (0, 2e-6, 0), (40000, 0, 0), (np.inf, -np.inf, 0)]
        for i, at in enumerate(idx):
            flat[at, :3] = rows[i % len(rows)]
    return scene.view(np.uint16)
