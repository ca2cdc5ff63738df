"""numpy restatement of the mip-chain generator (include/sah_mip_chain.h), written from the shader text thread by thread:
RenderCore/extern/spd/ffx_spd.h:855-1283 (SpdDownsampleH, the packed path with wave operations) as the four shaders
RenderCore/shaders/util/mip_chain_generator_*.comp instantiate it.  One workgroup after the other in dispatch order; inside a workgroup
every array below has one entry per thread (256), `x` / `y` come from ARmpRed8x8, the quad exchanges are index permutations tid ^ 1, ^ 2,
^ 3, `mid` is spdIntermediate[16][16] with the shader's own addresses, and `counter` is the global atomic.  Every half operator is one
numpy float16 operation and every fp32 operator one float32 operation, so each is rounded on its own; fma is exact (fma32).  Test
infrastructure only; parity unpinned.  tools/gen_golden_mip_chain.py holds a second, geometric restatement that must agree."""
import numpy as np

f16, f32 = np.float16, np.float32
FORMAT_R16, FORMAT_RGBA16, FORMAT_R32, FORMAT_B10G11R11, FORMAT_D32 = 76, 97, 100, 122, 126
# source format -> (destination format, channels carried, reduction)
PAIRS = {FORMAT_D32: (FORMAT_R32, 1, "min"), FORMAT_R32: (FORMAT_R32, 1, "min"), FORMAT_R16: (FORMAT_R16, 1, "mean"),
         FORMAT_RGBA16: (FORMAT_RGBA16, 4, "mean"), FORMAT_B10G11R11: (FORMAT_B10G11R11, 3, "mean")}
STORAGE = {FORMAT_R32: np.uint32, FORMAT_D32: np.uint32, FORMAT_R16: np.uint16, FORMAT_RGBA16: np.uint16, FORMAT_B10G11R11: np.uint32}


def fma32(a, b, c):
    """fl32(a * b + c), one rounding.  The product of two fp32 values is exact in fp64; the fp64 sum is made round-to-odd with the exact
    error of the addition (TwoSum), and a round-to-odd value of 53 bits rounds to 24 bits as the exact sum would."""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        odd = (np.ascontiguousarray(s).view(np.int64) & 1) == 1
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def spd_mips(w, h):
    """SpdSetup, ffx_spd.h:348-349"""
    return int(min(np.floor(np.log2(f32(max(w, h)))), 12))


def hi_z_extent_and_levels(resolution):
    """DepthCullingPhase::set_render_resolution, depth_culling_phase.cpp:96-98: resolution / 2 and round(log2(float(major dimension)))"""
    w, h = resolution[0] // 2, resolution[1] // 2
    return (w, h), int(np.round(np.log2(f32(max(w, h)))))


def level_extents(extent0, n):
    return [(max(1, extent0[0] >> i), max(1, extent0[1] >> i)) for i in range(n)]


def armp_red8x8(a):
    """ffx_a.h: x = a0 + 2 a3 + 4 a4, y = a1 + 2 a2 + 4 a5"""
    return (a & 1) | ((a >> 2) & 6), ((a >> 1) & 3) | ((a >> 3) & 4)


# ---- formats ------------------------------------------------------------------------------------------------------------------------------
def decode(bits, fmt):
    """storage -> float16 (..., C)"""
    bits = np.asarray(bits)
    if fmt in (FORMAT_R32, FORMAT_D32):
        with np.errstate(all="ignore"):
            return np.ascontiguousarray(bits).view(f32).astype(f16)[..., None]
    if fmt == FORMAT_R16:
        return np.ascontiguousarray(bits).view(f16)[..., None]
    if fmt == FORMAT_RGBA16:
        return np.ascontiguousarray(bits).view(f16)
    w = bits.astype(np.uint32)
    h = np.stack([(w & 0x7ff) << 4, ((w >> 11) & 0x7ff) << 4, ((w >> 22) & 0x3ff) << 5], axis=-1).astype(np.uint16)
    return h.view(f16)


def source_values(src, fmt):
    """what the sampler fetches: fp32 (H, W, C); an fp32 source is NOT rounded to half first"""
    if fmt in (FORMAT_R32, FORMAT_D32):
        return np.ascontiguousarray(src).view(f32)[..., None]
    return decode(src, fmt).astype(f32)


def encode(v, fmt):
    """float16 (..., C) -> storage"""
    v = np.ascontiguousarray(v, f16)
    if fmt == FORMAT_R32:
        return v[..., 0].astype(f32).view(np.uint32)
    if fmt == FORMAT_R16:
        return v[..., 0].view(np.uint16)
    if fmt == FORMAT_RGBA16:
        return v.view(np.uint16)
    hb = v.view(np.uint16).astype(np.uint32)

    def uf(h, shift, nan_code):  # the library's encoder (csrc/r11g11b10.hpp) on a half: NaN canonical, negatives 0, else truncation
        nan = (h & 0x7fff) > 0x7c00
        return np.where(nan, nan_code, np.where(h & 0x8000, 0, (h & 0x7fff) >> shift)).astype(np.uint32)
    return uf(hb[..., 0], 4, 0x7e0) | (uf(hb[..., 1], 4, 0x7e0) << 11) | (uf(hb[..., 2], 5, 0x3f0) << 22)


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------
def hmin(a, b):
    """minNum on halves: a NaN operand yields the other; -0 orders below +0"""
    with np.errstate(all="ignore"):
        take_b = np.isnan(a) | (b < a) | ((a == b) & np.signbit(b))
        return np.where(take_b & ~np.isnan(b), b, a)


def reduce4(v0, v1, v2, v3, how):
    if how == "min":
        return canonical(hmin(hmin(v0, v1), hmin(v2, v3)))
    with np.errstate(all="ignore"):
        return canonical((((v0 + v1) + v2) + v3) * f16(0.25))


def sample(img, tx, ty):
    """SpdLoadSourceImageH: LINEAR / REPEAT at texcoord = tex * inv + inv, then AH4(): float16 (N, C)"""
    h, w = img.shape[:2]

    def axis(t, n):
        inv = f32(1) / f32(n)
        u = t.astype(f32) * inv + inv
        p = u * f32(n) - f32(0.5)
        p0 = np.floor(p)
        i = p0.astype(np.int64)
        return i % n, (i + 1) % n, (p - p0).astype(f32)
    xa, xb, fx = axis(np.asarray(tx), w)
    ya, yb, fy = axis(np.asarray(ty), h)
    wx0, wy0 = f32(1) - fx, f32(1) - fy
    acc = fma32((wx0 * wy0)[:, None], img[ya, xa], f32(0))
    acc = fma32((fx * wy0)[:, None], img[ya, xb], acc)
    acc = fma32((wx0 * fy)[:, None], img[yb, xa], acc)
    acc = fma32((fx * fy)[:, None], img[yb, xb], acc)
    with np.errstate(all="ignore"):
        return canonical(acc.astype(f16))


def canonical(v):
    """NaNs as the GPU makes them: the positive quiet NaN 0x7e00.  (The host's arithmetic under numpy produces the negative one for an
    invalid operation; which NaN comes out is not what this restatement is about.)"""
    v = np.array(v, f16)
    v.view(np.uint16)[np.isnan(v)] = 0x7e00
    return v


# ---- the shader ---------------------------------------------------------------------------------------------------------------------------
class _Run:
    def __init__(self, src, src_format, extent0, num_levels, init):
        self.dst_format, self.C, self.how = PAIRS[src_format]
        self.img = source_values(src, src_format)
        self.H, self.W = self.img.shape[:2]
        self.n = num_levels
        self.mips = spd_mips(self.W, self.H)
        self.bounds = level_extents(extent0, 12)  # what bounds a store to slot i: the extent level i has or would have
        shape = (lambda w, h: (h, w, 4) if self.dst_format == FORMAT_RGBA16 else (h, w))
        if init is None:
            self.levels = [np.zeros(shape(w, h), STORAGE[self.dst_format]) for w, h in self.bounds[:num_levels]]
        else:
            self.levels = [np.array(a, STORAGE[self.dst_format]) for a in init]
        self.mid = np.zeros((16, 16, self.C), f16)
        self.counter = 0

    def store(self, slot, px, py, v, active=None):
        """SpdStoreH: imageStore(imgDst[slot], ...) — slots from num_levels on are level 1's view; dropped outside the extent"""
        w, h = self.bounds[slot]
        ok = (px < w) & (py < h)
        if active is not None:
            ok &= active
        target = self.levels[slot if slot < self.n else 1]
        target[py[ok], px[ok]] = encode(v[ok], self.dst_format)

    def load5(self, px, py):
        """SpdLoadH: imageLoad(imgDst[5], p), 0 outside"""
        w, h = self.bounds[5]
        ok = (px < w) & (py < h)
        out = np.zeros((len(px), self.C), f16)
        out[ok] = decode(self.levels[5][py[ok], px[ok]], self.dst_format)
        return out

    def reduce_quad(self, v):
        t = np.arange(len(v))
        return reduce4(v, v[t ^ 1], v[t ^ 2], v[t ^ 3], self.how)

    def next_four(self, x, y, wx, wy, tid, base):
        """SpdDownsampleNextFourH :1239-1256 (a barrier in front of every stage)"""
        mid, q0 = self.mid, (tid % 4) == 0
        if self.mips <= base:
            return
        v = self.reduce_quad(mid[x, y])
        self.store(base, wx * 8 + x // 2, wy * 8 + y // 2, v, q0)
        mid[(x + (y // 2) % 2)[q0], y[q0]] = v[q0]
        if self.mips <= base + 1:
            return
        a = tid < 64
        xs, ys, qs = x[a], y[a], q0[a]
        v = self.reduce_quad(mid[xs * 2 + ys % 2, ys * 2])
        self.store(base + 1, wx * 4 + xs // 2, wy * 4 + ys // 2, v, qs)
        mid[(xs * 2 + ys // 2)[qs], (ys * 2)[qs]] = v[qs]
        if self.mips <= base + 2:
            return
        a = tid < 16
        xs, ys, qs = x[a], y[a], q0[a]
        v = self.reduce_quad(mid[xs * 4 + ys, ys * 4])
        self.store(base + 2, wx * 2 + xs // 2, wy * 2 + ys // 2, v, qs)
        mid[(xs // 2 + ys)[qs], 0] = v[qs]
        if self.mips <= base + 3:
            return
        v = self.reduce_quad(mid[np.arange(4), 0])
        self.store(base + 3, np.array([wx]), np.array([wy]), v[:1])

    def workgroup(self, wx, wy, num_workgroups):
        tid = np.arange(256)
        sx, sy = armp_red8x8(tid % 64)
        x, y = sx + 8 * ((tid >> 6) % 2), sy + 8 * (tid >> 7)
        # SpdDownsampleMips_0_1_IntrinsicsH :956-1002
        v = []
        for q in range(4):
            ox, oy = 16 * (q & 1), 16 * (q >> 1)
            v.append(sample(self.img, wx * 64 + 2 * (x + ox), wy * 64 + 2 * (y + oy)))
            self.store(0, wx * 32 + x + ox, wy * 32 + y + oy, v[q])
        if self.mips <= 1:
            return
        q0 = (tid % 4) == 0
        for q in range(4):
            ox, oy = 8 * (q & 1), 8 * (q >> 1)
            r = self.reduce_quad(v[q])
            self.store(1, wx * 16 + x // 2 + ox, wy * 16 + y // 2 + oy, r, q0)
            self.mid[(x // 2 + ox)[q0], (y // 2 + oy)[q0]] = r[q0]
        self.next_four(x, y, wx, wy, tid, 2)
        if self.mips < 7:
            return
        # SpdExitWorkgroup :1273-1277
        ticket = self.counter
        self.counter += 1
        if ticket != num_workgroups - 1:
            return
        self.counter = 0
        # SpdDownsampleMips_6_7H :1209-1237
        w = []
        for q in range(4):
            tx, ty = x * 4 + 2 * (q & 1), y * 4 + 2 * (q >> 1)
            w.append(reduce4(self.load5(tx, ty), self.load5(tx, ty + 1), self.load5(tx + 1, ty), self.load5(tx + 1, ty + 1), self.how))
            self.store(6, x * 2 + (q & 1), y * 2 + (q >> 1), w[q])
        if self.mips < 8:
            return
        r = reduce4(w[0], w[1], w[2], w[3], self.how)
        self.store(7, x, y, r)
        self.mid[x, y] = r
        self.next_four(x, y, 0, 0, tid, 8)


def generate(src, src_format, extent0, num_levels, init=None):
    """The levels after sah_mip_chain_generate, as storage bit patterns (uint32 (h, w) for R32 and B10G11R11, uint16 (h, w) for R16,
    uint16 (h, w, 4) for RGBA16F).  src: the source's storage array (float32 or uint32 for D32 / R32); extent0: (w0, h0) of level 0;
    init: the levels' contents before the call (default zeros).  The call must be one the entry point accepts."""
    run = _Run(src, src_format, extent0, num_levels, init)
    gx, gy = (run.W + 63) // 64, (run.H + 63) // 64
    for wy in range(gy):
        for wx in range(gx):
            run.workgroup(wx, wy, gx * gy)
    assert run.counter == 0
    return run.levels
