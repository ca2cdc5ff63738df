"""Writes tests/golden/mip_chain_160x96.npz and mip_chain_192x136.npz: one source per format pair of sah_mip_chain_generate
(include/sah_mip_chain.h) and the levels the call leaves — 160 x 96 into 80 x 48 with 6 levels (SPD makes 7: the stray store into level 1),
192 x 136 into 96 x 68 with 7 levels (9 workgroups, odd level extents).

    python tools/gen_golden_mip_chain.py

The levels are computed twice, by two restatements that share no code, and written only when they agree bit for bit: tests/mip_chain_ref.py
follows the shader thread by thread; `chain()` below is written geometrically — for each level and texel it names which four values of the
level above are reduced, in which order, and whether those are HELD values (what a workgroup computed, stored or not) or STORED ones.

Inputs (seeded): depth is reversed-Z, near / distance over smooth random distances, with a sky region of exact zeros, a region of fp16-
subnormal depths, a region of fp32 values that lie halfway between two halves, one +inf and one NaN.  Colour covers the whole half range
in exponent — subnormals to 65504 — with both signs for the signed formats; negative values stay below 16000 in magnitude so that no sum
reaches -inf (+inf minus -inf would be a NaN whose sign is the adder's business), and a region of values 1 + k / 1024 makes the sums tie."""
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f16, f32 = np.float16, np.float32
D32, R32, R16, RGBA16, B10G11R11 = 126, 100, 76, 97, 122
NAMES = {D32: "d32", R16: "r16", RGBA16: "rgba16", B10G11R11: "b10g11r11"}
CASES = {"160x96": ((160, 96), (80, 48), 6), "192x136": ((192, 136), (96, 68), 7)}
SEED = 5
PLANTED = {"inf": (40, 30), "nan": (100, 70)}  # (x, y) in the depth sources


def fixture_path(tag):
    return os.path.join(ROOT, "tests", "golden", f"mip_chain_{tag}.npz")


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _half_bits(g, shape, signed):
    """halves over the whole exponent range: a uniform exponent field 0..30 with a random mantissa"""
    bits = (g.integers(0, 31, shape).astype(np.uint16) << 10) | g.integers(0, 1024, shape).astype(np.uint16)
    if signed:
        neg = (g.random(shape) < 0.3) & (bits.view(f16) < 16000)
        bits = bits | (neg.astype(np.uint16) << 15)
    return bits


def inputs(size, seed=SEED):
    w, h = size
    g = np.random.default_rng(seed + w)
    yy, xx = np.mgrid[0:h, 0:w]
    dist = (0.3 + 40.0 * g.random((h, w)) ** 3 * (1 + yy / h)).astype(f32)
    depth = (f32(0.05) / dist).astype(f32)
    depth[: h // 5, w // 2:] = 0                                                          # sky
    sub = g.uniform(1e-7, 6e-5, (h // 4, w // 4)).astype(f32)
    depth[h // 2: h // 2 + h // 4, : w // 4] = sub                                        # fp16 subnormals (below 2^-14)
    k = g.integers(0x2000, 0x3c00, (h // 4, w // 4)).astype(np.uint16)                    # halves in [2^-7, 1) ...
    depth[h // 2: h // 2 + h // 4, w // 2: w // 2 + w // 4] = np.repeat(np.repeat(      # ... plus half an ulp, constant over 4 x 4 source texels
        (k.view(f16).astype(f32).view(np.uint32) | 0x1000).view(f32)[: h // 16 + 1, : w // 16 + 1], 4, 0), 4, 1)[: h // 4, : w // 4]
    bits = depth.view(np.uint32)
    bits[PLANTED["inf"][1], PLANTED["inf"][0]] = 0x7f800000
    bits[PLANTED["nan"][1], PLANTED["nan"][0]] = 0x7fc00000
    out = {D32: depth}
    r16 = _half_bits(g, (h, w), True)
    rgba = _half_bits(g, (h, w, 4), True)
    ties = (f16(1) + g.integers(0, 1024, (h // 4, w // 4)).astype(f16) / f16(1024)).view(np.uint16)
    r16[: h // 4, : w // 4] = ties
    rgba[: h // 4, : w // 4] = ties[..., None]
    packed = _half_bits(g, (h, w, 3), False).astype(np.uint32)
    out[R16], out[RGBA16] = r16, rgba
    out[B10G11R11] = (packed[..., 0] >> 4) | ((packed[..., 1] >> 4) << 11) | ((packed[..., 2] >> 5) << 22)
    return out


# ---- the geometric restatement ------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl32(a * b + c) for fp32 arrays.  The product is exact in fp64; where the fp64 sum is exact too its rounding to fp32 is the fma's, and
    the other elements are redone in rational arithmetic."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        t = s - p
        exact = ~np.isfinite(s) | (((p - (s - t)) + (c - t)) == 0)  # the addition's exact error (TwoSum)
        out = s.astype(f32)
    for i in zip(*np.nonzero(~exact)):
        r = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = f32(float(s[i]))  # a neighbour of the result; walk to the nearest, ties to even
        cands = sorted({float(np.nextafter(lo, f32(-np.inf))), float(lo), float(np.nextafter(lo, f32(np.inf)))})
        best = min(cands, key=lambda v: (abs(Fraction(v) - r), int(f32(v).view(np.uint32)) & 1))
        out[i] = f32(best)
    return out


def _to_half_values(src, fmt):
    """the texel values the sampler sees, fp32 (H, W, C)"""
    if fmt in (D32, R32):
        return np.ascontiguousarray(src).view(f32)[..., None]
    if fmt == R16:
        return np.ascontiguousarray(src).view(f16).astype(f32)[..., None]
    if fmt == RGBA16:
        return np.ascontiguousarray(src).view(f16).astype(f32)
    w = np.asarray(src, np.uint32)
    return np.stack([((w & 0x7ff) << 4).astype(np.uint16).view(f16), (((w >> 11) & 0x7ff) << 4).astype(np.uint16).view(f16),
                     (((w >> 22) & 0x3ff) << 5).astype(np.uint16).view(f16)], -1).astype(f32)


def _quiet(v):
    v = np.array(v, f16)
    v.view(np.uint16)[np.isnan(v)] = 0x7e00
    return v


def _reduce(a, b, c, d, minimum):
    with np.errstate(all="ignore"):
        if not minimum:
            return _quiet((((a + b) + c) + d) * f16(0.25))

        def lo(p, q):  # the smaller, a number before a NaN, -0 before +0
            r = np.fmin(p, q)
            return np.where((p == 0) & (q == 0) & (np.signbit(p) | np.signbit(q)), f16(-0.0), r)
        return _quiet(lo(lo(a, b), lo(c, d)))


def _pack(v, fmt):
    v = np.ascontiguousarray(v, f16)
    if fmt == R32:
        return v[..., 0].astype(f32).view(np.uint32)
    if fmt == R16:
        return v[..., 0].view(np.uint16).copy()
    if fmt == RGBA16:
        return v.view(np.uint16).copy()
    b = v.view(np.uint16).astype(np.uint32)
    nan, neg, mag = (b & 0x7fff) > 0x7c00, (b & 0x8000) != 0, b & 0x7fff
    r = np.where(nan[..., 0], 0x7e0, np.where(neg[..., 0], 0, mag[..., 0] >> 4))
    g = np.where(nan[..., 1], 0x7e0, np.where(neg[..., 1], 0, mag[..., 1] >> 4))
    bl = np.where(nan[..., 2], 0x3f0, np.where(neg[..., 2], 0, mag[..., 2] >> 5))
    return (r | (g << 11) | (bl << 22)).astype(np.uint32)


def _unpack(bits, fmt):
    if fmt == R32:
        with np.errstate(all="ignore"):
            return np.ascontiguousarray(bits).view(f32).astype(f16)[..., None]
    return _to_half_values(bits, fmt).astype(f16)


def chain(src, src_format, extent0, num_levels):
    """The levels sah_mip_chain_generate leaves in an image that held zeros.

    HELD level 0: one sample per texel of the grid the workgroups cover, 32 ceil(W / 64) x 32 ceil(H / 64), whether the image has that texel
    or not.  HELD level k, k = 1 .. 5: the reduction of the 2 x 2 block of HELD level k - 1 in the order own, right, below, diagonal (tiles are
    32 texels wide at level 0, so a block never straddles two workgroups).  STORED level k: HELD level k cut to the level's extent.
    HELD level 6: 32 x 32 reductions over STORED level 5 padded with zeros to 64 x 64, in the order own, BELOW, RIGHT, diagonal.
    HELD level k, k = 7 .. 11: own, right, below, diagonal of HELD level k - 1.
    A level i >= num_levels is stored into level 1 instead, cut to the extent level i would have; levels >= 6 land after every other store,
    in level order."""
    dst_format = R32 if src_format in (D32, R32) else src_format
    minimum = dst_format == R32
    img = _to_half_values(src, src_format)
    H, W = img.shape[:2]
    mips = int(min(np.floor(np.log2(f32(max(W, H)))), 12))
    made = max(mips, 1)
    GW, GH = 32 * ((W + 63) // 64), 32 * ((H + 63) // 64)
    # held level 0
    ys, xs = np.mgrid[0:GH, 0:GW]

    def axis(t, n):
        inv = f32(1) / f32(n)
        p = ((f32(2) * t.astype(f32)) * inv + inv) * f32(n) - f32(0.5)
        fl = np.floor(p)
        return fl.astype(np.int64) % n, (fl.astype(np.int64) + 1) % n, (p - fl).astype(f32)
    x0, x1, fx = axis(xs, W)
    y0, y1, fy = axis(ys, H)
    gx, gy = f32(1) - fx, f32(1) - fy
    acc = _fma((gx * gy)[..., None], img[y0, x0], f32(0))
    acc = _fma((fx * gy)[..., None], img[y0, x1], acc)
    acc = _fma((gx * fy)[..., None], img[y1, x0], acc)
    acc = _fma((fx * fy)[..., None], img[y1, x1], acc)
    with np.errstate(all="ignore"):
        held = [_quiet(acc.astype(f16))]
    for k in range(1, min(made, 6)):
        a = held[-1]
        held.append(_reduce(a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2], minimum))
    extents = [(max(1, extent0[0] >> i), max(1, extent0[1] >> i)) for i in range(12)]
    shape = (lambda w, h: (h, w, 4) if dst_format == RGBA16 else (h, w))
    levels = [np.zeros(shape(*extents[i]), np.uint32 if dst_format in (R32, B10G11R11) else np.uint16) for i in range(num_levels)]

    def put(i, values):
        w, h = extents[i]
        cut = values[:h, :w]
        levels[i if i < num_levels else 1][:cut.shape[0], :cut.shape[1]] = _pack(cut, dst_format)
    for i in [k for k in range(len(held)) if k < num_levels] + [k for k in range(len(held)) if k >= num_levels]:
        put(i, held[i])  # (missing levels below 6 only ever come from one workgroup, after its own level 1)
    if made >= 7:
        w5, h5 = extents[5]
        stored5 = np.zeros((64, 64, img.shape[2]), f16)
        stored5[:min(h5, 64), :min(w5, 64)] = _unpack(levels[5], dst_format)[:64, :64]
        a = stored5
        held.append(_reduce(a[0::2, 0::2], a[1::2, 0::2], a[0::2, 1::2], a[1::2, 1::2], minimum))
        put(6, held[6])
        for k in range(7, made):
            a = held[-1]
            held.append(_reduce(a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2], minimum))
            put(k, held[k])
    return levels


def generate(tag, seed=SEED):
    sys.path.insert(0, ROOT)
    from tests import mip_chain_ref
    size, extent0, n = CASES[tag]
    out = {"seed": np.int64(seed), "extent0": np.array(extent0, np.uint32), "num_levels": np.int64(n)}
    for fmt, src in inputs(size, seed).items():
        a = chain(src, fmt, extent0, n)
        b = mip_chain_ref.generate(src, fmt, extent0, n)
        for i in range(n):
            assert a[i].dtype == b[i].dtype and a[i].tobytes() == b[i].tobytes(), f"{tag} {NAMES[fmt]}: the two restatements differ at level {i}"
        out[f"{NAMES[fmt]}_src"] = src
        for i in range(n):
            out[f"{NAMES[fmt]}_level{i}"] = a[i]
    return out


if __name__ == "__main__":
    for tag in CASES:
        out = generate(tag)
        np.savez_compressed(fixture_path(tag), **out)
        print(f"{fixture_path(tag)}: {os.path.getsize(fixture_path(tag))} bytes")
