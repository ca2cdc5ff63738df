"""Vectorised numpy restatement of the two VRSAA shaders (include/sah_vrsaa.h), written from the shader text:
RenderCore/shaders/vrsaa/contrast_detection.comp:15-68 and generate_shading_rate_image.comp:19-63.  Every operator is one float32 numpy
operation, so each is rounded on its own.  Test infrastructure only; parity unpinned (the reference ships no images of these passes).
tools/gen_golden_vrsaa.py writes the fixture with it; tests/test_vrsaa_cpu.py holds a second, scalar restatement that must agree."""
import numpy as np

f32 = np.float32
RATES = [(1, 1), (1, 2), (2, 1), (2, 2), (2, 4), (4, 2), (4, 4)]  # the seven rates of the fixture
# contrast_detection.comp:23-33, column-major mat3 constructors: M[column][row], and the shader indexes [x][y]
SOBEL_X = [[1, 0, -1], [2, 0, -2], [1, 0, -1]]
SOBEL_Y = [[1, 2, 1], [0, 0, 0], [-1, -2, -1]]


def srgb_lut():
    """sRGB8 -> linear, the Vulkan EOTF in double rounded to fp32 (the library's table, api.cpp: sah_create)"""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(f32)


def maxnum(a, b):  # oracle/math.hpp:59
    return np.where((a < b) | np.isnan(a), b, a)


def minnum(a, b):
    return np.where((b < a) | np.isnan(a), b, a)


def nearest_index(n):
    """Texel index of the NEAREST / CLAMP_TO_EDGE sampler for texcoord float(s) / n, s = -1 .. n (entry k is s = k - 1): the rule of
    oracle/texture.hpp:39-43, floor(uv * n) clamped."""
    s = np.arange(-1, n + 1, dtype=np.int64)
    uv = s.astype(f32) / f32(n)
    return np.clip(np.floor(uv * f32(n)).astype(np.int64), 0, n - 1)


def low_landing(n):
    """the s in [0, n) whose tap lands on texel s - 1"""
    idx = nearest_index(n)[1:-1]
    assert ((idx == np.arange(n)) | (idx == np.arange(n) - 1)).all()
    return [int(s) for s in np.nonzero(idx < np.arange(n))[0]]


def luma(color):
    """color: (H, W, 4) uint8, R8G8B8A8_SRGB"""
    lut = srgb_lut()
    r, g, b = lut[color[..., 0]], lut[color[..., 1]], lut[color[..., 2]]
    return (r * f32(0.2126) + g * f32(0.7152)) + b * f32(0.0722)


def gradients(v):
    """the two Sobel sums of an (H, W) float32 plane, taps through the sampler: (H, W, 2) float32"""
    h, w = v.shape
    xi, yi = nearest_index(w), nearest_index(h)
    gx, gy = np.zeros((h, w), f32), np.zeros((h, w), f32)
    with np.errstate(all="ignore"):
        for y in range(3):
            for x in range(3):
                t = v[yi[y:y + h, None], xi[None, x:x + w]]  # s = p + (x, y) - 1 is entry p + (x, y) of the maps
                gx = gx + t * f32(SOBEL_X[x][y])
                gy = gy + t * f32(SOBEL_Y[x][y])
    return np.stack([gx, gy], -1)


def contrast(color, depth):
    """(H, W, 2) uint16: the R16G16_SFLOAT contrast image"""
    with np.errstate(all="ignore"):
        out = maxnum(gradients(luma(color)) * f32(0.5), gradients(np.ascontiguousarray(depth, f32)))
        return np.ascontiguousarray(out.astype(np.float16)).view(np.uint16)


def block_size(cw, sw):
    return max(1, int(np.rint(f32(cw) / f32(sw))))  # np.rint: ties to even


def rate_code(rx, ry):
    return ((ry >> 1) | ((rx << 1) & 12)) & 0xff


def shading_rate_image(contrast_bits, sri_extent, rates, num_rates=None, max_rate=None):
    """contrast_bits: (H, W, 2) uint16; sri_extent: (width, height); rates: up to eight (x, y); num_rates / max_rate default to what
    scene.shading_rate_params fills in.  Returns (height, width) uint8."""
    ch, cw = contrast_bits.shape[:2]
    sw, sh = sri_extent
    table = [(int(x), int(y)) for x, y in rates] + [(0, 0)] * (8 - len(rates))
    n = len(rates) if num_rates is None else num_rates
    if max_rate is None:
        max_rate = (max([r[0] for r in rates], default=0), max([r[1] for r in rates], default=0))
    d = block_size(cw, sw)
    g = contrast_bits.view(np.float16).astype(f32)
    px, py = np.meshgrid(np.arange(sw, dtype=np.int64), np.arange(sh, dtype=np.int64))
    m = np.zeros((sh, sw, 2), f32)
    with np.errstate(all="ignore"):
        for i in range(d):
            for j in range(d):
                x, y = d * px + i, d * py + j
                inside = (x < cw) & (y < ch)
                t = np.where(inside[..., None], g[np.minimum(y, ch - 1), np.minimum(x, cw - 1)], f32(0))
                m = maxnum(m, np.abs(t * t))
        a = minnum(f32(1.25) * np.sqrt(m), f32(1))
        R = f32(max(max_rate))
        opt = a * f32(1) + (f32(1) - a) * R
        best = np.zeros((sh, sw), np.int64)
        cost = np.full((sh, sw), f32(1) + (f32(2) * R) * R, f32)
        for k in range(n):
            dx, dy = f32(table[k][0]) - opt[..., 0], f32(table[k][1]) - opt[..., 1]
            c = dx * dx + dy * dy
            take = c < cost
            cost = np.where(take, c, cost)
            best = np.where(take, k, best)
    codes = np.array([rate_code(x, y) for x, y in table], np.uint8)
    return codes[best]
