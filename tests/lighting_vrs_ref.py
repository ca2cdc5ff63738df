"""numpy restatement of include/sah_vrs.h: the source map of sah_lighting_vrs and the arithmetic of sah_vrsaa_resolve, with explicit
np.float32 operations; and the inputs of the parity cases (tests/test_lighting_vrs_cpu.py shows that they are not vacuous,
tests/test_lighting_vrs_gpu.py runs them)."""
import numpy as np

f32 = np.float32

# Vulkan's code of a rate (w, h): (log2 w << 2) | log2 h — the seven rates sah_vrsaa_shading_rate_image chooses among (tests/vrsaa_ref.py: RATES)
RATE_CODES = {(1, 1): 0, (1, 2): 1, (2, 1): 4, (2, 2): 5, (2, 4): 6, (4, 2): 9, (4, 4): 10}


def rate_of(code):
    """(lw, lh): log2 of the coarse pixel's extent — a field value of 3 counts as 2, bits 4-7 are ignored"""
    code = int(code)
    return min((code >> 2) & 3, 2), min(code & 3, 2)


def source_map(depth, rate_image, texel_size, tol):
    """(sy, sx): the pixel whose sah_lighting value pixel (y, x) receives"""
    d = np.ascontiguousarray(depth, f32)
    h, w = d.shape
    tx, ty = texel_size
    tol = f32(tol)
    surface = d != f32(0.0)  # NaN is a surface, -0 is not
    sy, sx = (a.copy() for a in np.mgrid[0:h, 0:w])
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if not surface[y, x]:
                    continue
                lw, lh = rate_of(rate_image[y // ty, x // tx])
                ox, oy = x & ~((1 << lw) - 1), y & ~((1 << lh) - 1)
                box = surface[oy:min(oy + (1 << lh), h), ox:min(ox + (1 << lw), w)]
                first = int(np.argmax(box.reshape(-1)))  # row-major; the box holds (y, x), so one exists
                ry, rx = oy + first // box.shape[1], ox + first % box.shape[1]
                dq, dr = d[y, x], d[ry, rx]
                if np.abs(f32(dq - dr)) <= f32(tol * np.abs(dr)):  # a NaN compares false
                    sy[y, x], sx[y, x] = ry, rx
    return sy, sx


def resolve(lit_halfs, rows=(0, 0)):
    """lit_halfs (2H, 2W, 4) uint16 -> rows [begin, end) of the (H, W, 4) uint16 resolve ((0, 0) = all)"""
    lit = np.ascontiguousarray(lit_halfs, np.uint16)
    assert lit.shape[0] % 2 == 0 and lit.shape[1] % 2 == 0
    f = lit.view(np.float16).astype(f32)
    a, b, c, d = f[0::2, 0::2], f[0::2, 1::2], f[1::2, 0::2], f[1::2, 1::2]
    with np.errstate(all="ignore"):
        r = f32(0.25) * ((a + b) + (c + d))
        bits = r.astype(np.float16).view(np.uint16).copy()  # round to nearest even
    bits[np.isnan(r)] = 0x7e00
    r0, r1 = (0, bits.shape[0]) if tuple(rows) == (0, 0) else rows
    return bits[r0:r1]


# ---- the inputs of the parity cases -------------------------------------------------------------------------------------------------------
TOLERANCE = 0.01
# (width, height, texel size): partial 32 x 32 regions, partial texels and cut coarse pixels on both edges at 75 x 45; whole texels at 64 x 36;
# texels of 4 x 64 (the smallest and the largest) with both edges cut at 38 x 70
PARITY_CASES = [(75, 45, (8, 8)), (64, 36, (16, 16)), (38, 70, (4, 64))]
# the texels' codes in turn: mostly coarse, every one of the seven rates, fields of 3 (0x0f: 4 x 4, 0x07: 2 x 4) and high bits (0xf5: 2 x 2, 0xa0: 1 x 1)
CODE_CYCLE = [10, 5, 9, 6, 0x0f, 10, 4, 5, 1, 10, 0xf5, 0, 9, 0x07, 10, 5, 0xa0, 6]


def rate_image(w, h, texel_size, seed):
    """the codes of CODE_CYCLE over ceil(w / tx) x ceil(h / ty) texels; the last column and row 4 x 4, so that the edges cut coarse pixels"""
    sw, sh = -(-w // texel_size[0]), -(-h // texel_size[1])
    idx = (np.arange(sh)[:, None] * 7 + np.arange(sw)[None, :] + seed) % len(CODE_CYCLE)
    img = np.array(CODE_CYCLE, np.uint8)[idx]
    img[:, -1] = 10
    img[-1, :] = 0x0f
    return img


def block_depth(w, h, seed):
    """blocks of near-equal depth (relative steps of 1e-4 inside a block: within TOLERANCE) with sky holes — single pixels, first pixels of
    coarse pixels, whole 4 x 4 boxes — steps across blocks and inside them (a pixel at 1.5 x its block's depth: rejected), and one each of
    NaN, +inf, -inf and -0"""
    g = np.random.default_rng(seed)
    by, bx = -(-h // 8), -(-w // 8)
    base = (0.2 + 0.7 * g.random((by, bx))).astype(f32)
    d = np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w].copy()
    d *= (1.0 + 1e-4 * g.random((h, w))).astype(f32)
    d[g.random((h, w)) < 0.04] *= f32(1.5)   # steps inside a block
    d[g.random((h, w)) < 0.06] = 0.0         # sky holes
    d[0::4, 0::4][g.random(d[0::4, 0::4].shape) < 0.25] = 0.0  # a sky pixel in front of the representative
    for y, x in zip(g.integers(0, h // 4, 6) * 4, g.integers(0, w // 4, 6) * 4):
        d[y:y + 4, x:x + 4] = 0.0            # coarse pixels with no surface pixel
    d[-1, -1] = d[-2, -2] if d[-2, -2] != 0 else f32(0.5)  # a surface pixel in the corner's cut coarse pixel
    bits = d.view(np.uint32)
    for b in (0x7fc00000, 0x7f800000, 0xff800000, 0x80000000):
        bits[g.integers(0, h), g.integers(0, w)] = b
    return d


def parity_inputs(case):
    """(depth, rate image) of PARITY_CASES[case]"""
    w, h, texel = PARITY_CASES[case]
    return block_depth(w, h, 900 + case), rate_image(w, h, texel, case)
