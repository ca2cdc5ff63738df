"""numpy restatement of sah_taa_upscale (include/sah_taa_upscale.h), step for step and bit for bit: fp32 operators throughout, the two fma
chains (history tap, upsample) through tests/mip_chain_ref.fma32, and Bounds / Motion through tests/taa_ref.py's own functions applied to
the render planes and gathered at each output pixel's nearest texel."""
import numpy as np

from tests.mip_chain_ref import fma32
from tests.taa_ref import HDR_WEIGHTS, HISTORY_INVALID, dilated_texel, fmax, fmin, jitter_cycle, neighbourhood

f32 = np.float32
TILE = (64, 16)        # the kernel's tile of `out` (androidrenderer_amd/csrc/taa_upscale.hip)
FOOTPRINT = (67, 19)   # the cells of the render planes it stages at most: nearest texels of the tile's first to last pixel plus a halo of one
# (render (w, h), output (W, H)) of the small-extent GPU test; tests/test_taa_upscale_cpu.py checks the footprint bound over the same list
EXTENTS = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((1, 1), (256, 16)), ((64, 16), (64, 16)), ((64, 16), (65, 17)), ((65, 17), (129, 33)),
           ((65, 17), (130, 34)),  # exactly 2 x: with a jitter of 0.25, u lands on integers
           ((64, 36), (96, 54)), ((77, 36), (100, 37)), ((9, 1), (20, 1)), ((1, 9), (1, 20))]


def _rgb(bits):
    return np.ascontiguousarray(bits).view(np.float16)[..., :3].astype(f32)


def floor_to_int(v):
    """int(floor(v)) with the float saturated to [-2^31, 2^31 - 128] first (a NaN goes to the lower end, as fmax / fmin leave it)"""
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(np.floor(v), nan=-2147483648.0, posinf=2147483520.0, neginf=-2147483648.0), -2147483648.0, 2147483520.0).astype(np.int64)


def sample_positions(n_out, n_render, jitter, first=0, count=None):
    """(u, i): u = (float(X) + 0.5) * fl(n_render / n_out) - jitter for X in [0, n_out) — or for `count` pixels from `first` — and the nearest
    texel clamp(floor(u), 0, n_render - 1)"""
    s = f32(n_render) / f32(n_out)
    u = (np.arange(first, n_out if count is None else first + count).astype(f32) + f32(0.5)) * s - f32(jitter)
    assert u.dtype == f32
    return u, np.clip(floor_to_int(u), 0, n_render - 1)


def bilinear_axis(q, n):
    """one axis of the library's bilinear rule at pixel coordinate q over n texels: -> (a, b the two clamped taps, f the weight of b)"""
    with np.errstate(all="ignore"):
        p = np.asarray(q, f32) - f32(0.5)
        i0 = floor_to_int(p)
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), p - np.floor(p)


def bilinear(rgb, qx, qy, rows=None):
    """the library's bilinear rule at pixel coordinates over the float32 image rgb (h, w, 3): -> (value, (ya, yb, xa, xb) the clamped taps).
    rows = (first, height): rgb holds the rows from `first` on of an image of that height (the taps must fall inside it)"""
    h, w = rgb.shape[:2]
    first, height = (0, h) if rows is None else rows
    with np.errstate(all="ignore"):
        (xa, xb, fx), (ya, yb, fy) = bilinear_axis(qx, w), bilinear_axis(qy, height)
        ya, yb = ya - first, yb - first
        assert ya.min() >= 0 and yb.max() < h
        fx, fy = fx[..., None], fy[..., None]
        wx0, wy0 = f32(1) - fx, f32(1) - fy
        w00, w10, w01, w11 = wx0 * wy0, fx * wy0, wx0 * fy, fx * fy
        acc = fma32(w00, rgb[ya, xa], f32(0))
        acc = fma32(w10, rgb[ya, xb], acc)
        acc = fma32(w01, rgb[yb, xa], acc)
        return fma32(w11, rgb[yb, xb], acc), (ya, yb, xa, xb)


def _luma(v):
    return fmax((v[..., 0] * f32(0.2126) + v[..., 1] * f32(0.7152)) + v[..., 2] * f32(0.0722), f32(0.0))


def upscale_ex(lit, depth, mv, history, output, blend, min_confidence, jitter, previous_jitter, flags, window=None):
    """lit (h, w, 4), mv (h, w, 2) uint16, depth (h, w) float32, history (H, W, 4) uint16 or None, output = (W, H)
    -> (out (H, W, 4) uint16, info): i (W,), j (H,), u = (ux, uy), conf, q, in_range, history_finite, valid, fallback (no blended value
    stored), used_bilinear, used_nearest, upsample_taps, lo, hi, clamped.
    window = (Y0, rows, h0, h, history0), for images too high to restate whole: only rows [Y0, Y0 + rows) of the output are computed; lit,
    depth and mv hold the render rows from h0 on of planes h high, down to the last row, and history the rows from history0 on.  Every row
    a pixel of the window reads must lie inside the parts given, a row away from their upper end (asserted)."""
    lit = np.ascontiguousarray(lit).view(np.uint16)
    W, H = output
    Y0, rows, h0, h, history0 = (0, H, 0, depth.shape[0], 0) if window is None else window
    w = depth.shape[1]
    assert W >= w and H >= h and h0 + depth.shape[0] == h
    blend, min_confidence = f32(blend), f32(min_confidence)
    rx, ry = f32(W) / f32(w), f32(H) / f32(h)
    ux, i = sample_positions(W, w, jitter[0])
    uy, j_image = sample_positions(H, h, jitter[1], Y0, rows)
    j = j_image - h0  # (rows of the parts given)
    assert h0 == 0 or j.min() >= 2
    full_H, H = H, rows
    UX, UY = np.broadcast_to(ux[None, :], (H, W)), np.broadcast_to(uy[:, None], (H, W))
    nearest = lit[j][:, i]
    with np.errstate(all="ignore"):
        b, taps = bilinear(_rgb(lit), UX, UY, (h0, h))
        b_finite = np.isfinite(b).all(-1)
        b_bits = b.astype(np.float16).view(np.uint16)
    otherwise = np.where(b_finite[..., None], b_bits, nearest[..., :3])
    out = nearest.copy()
    info = {"i": i, "j": j_image, "u": (ux, uy), "upsample_taps": taps}
    if flags & HISTORY_INVALID:
        out[..., :3] = otherwise
        info.update(fallback=np.ones((H, W), bool), valid=np.zeros((H, W), bool), used_bilinear=b_finite, used_nearest=~b_finite)
        return out, info
    with np.errstate(all="ignore"):
        c = _rgb(nearest)
        lo, hi = (v[j][:, i] for v in neighbourhood(lit))
        by, bx = (v[j][:, i] for v in dilated_texel(depth))
        m = np.ascontiguousarray(mv).view(np.float16)[by, bx].astype(f32)
        dj = [f32(previous_jitter[0]) - f32(jitter[0]), f32(previous_jitter[1]) - f32(jitter[1])]
        qx = (np.arange(W).astype(f32)[None, :] + f32(0.5)) + (m[..., 0] + dj[0]) * rx
        qy = (np.arange(Y0, Y0 + H).astype(f32)[:, None] + f32(0.5)) + (m[..., 1] + dj[1]) * ry
        in_range = (qx >= 0) & (qx <= f32(W)) & (qy >= 0) & (qy <= f32(full_H))
        hv, _ = bilinear(_rgb(history), qx, qy, (history0, full_H))
        history_finite = np.isfinite(hv).all(-1)
        valid = in_range & history_finite
        hc = fmin(fmax(hv, lo), hi)
        ex = ((i.astype(f32) + f32(0.5)) - ux)[None, :] * rx
        ey = ((j_image.astype(f32) + f32(0.5)) - uy)[:, None] * ry
        t = np.minimum(ex * ex + ey * ey, f32(1))
        g = f32(1) - t
        conf = np.maximum(g * g, min_confidence)
        kb = blend * conf
        if flags & HDR_WEIGHTS:
            wc = kb / (f32(1) + _luma(c))
            wh = (f32(1) - kb) / (f32(1) + _luma(hc))
            k = wc / (wc + wh)
        else:
            k = kb
        o = hc + (c - hc) * k[..., None]
        assert o.dtype == f32 and conf.dtype == f32
        fallback = ~valid | ~np.isfinite(o).all(-1)
        o_bits = o.astype(np.float16).view(np.uint16)
    out[..., :3] = np.where(fallback[..., None], otherwise, o_bits)
    info.update(q=np.stack([qx, qy], -1), conf=conf, in_range=in_range, history_finite=history_finite, valid=valid, fallback=fallback,
                used_bilinear=fallback & b_finite, used_nearest=fallback & ~b_finite, lo=lo, hi=hi, h=hv,
                clamped=valid & ((hv < lo) | (hv > hi)).any(-1))
    return out, info


def upscale(lit, depth, mv, history, output, blend, min_confidence, jitter, previous_jitter, flags):
    return upscale_ex(lit, depth, mv, history, output, blend, min_confidence, jitter, previous_jitter, flags)[0]


def render_rows_read(row_begin, row_end, H, h, jitter_y):
    """[first, last] rows of lit, depth and motion_vectors that rows [row_begin, row_end) of `out` read"""
    _, j = sample_positions(H, h, jitter_y)
    return max(int(j[row_begin]) - 1, 0), min(int(j[row_end - 1]) + 1, h - 1)


# ---- the façade's TemporalUpscaling (include/sah_host.hpp) --------------------------------------------------------------------------------------
def render_resolution(output, scale):
    """max(1, uint32(float(W) / s + 0.5f)) per axis"""
    return tuple(max(1, int(f32(n) / f32(scale) + f32(0.5))) for n in output)


def jitter_phases(W, w):
    """ceil(8 W^2 / w^2), in integers"""
    return (8 * W * W + w * w - 1) // (w * w)


def upscale_jitter_cycle(W, w):
    return jitter_cycle(jitter_phases(W, w))
