"""fp64 reprojection of a pixel centre and its depth into the last frame — the check of tests/test_motion_vectors_gpu.py for geometry the
numpy restatement (tools/gen_golden_motion_vectors.py) cannot rasterise, and the measurement behind its tolerance."""
import numpy as np

# DESIGN.md §7 "Motion vectors", measured over the fixture's SOLID-won pixels between this reprojection and the bit-exact restatement
# (tests/test_motion_vectors_cpu.py recomputes both from the fixture).  The store rounds to half, which moves a value by up to half a
# spacing of the fp16 grid whatever computed it; what the fragment's interpolated position and the pixel-centre reprojection differ by
# beyond that — the 1/256-pixel snapping of the window triangle and the fp32 operators — is 0.00202 pixel at most.  In spacings of the
# fp16 grid at the stored value the same comparison reads 2871.7, because one component passes through zero: that unit bounds nothing
# away from zero, so both are applied.  Clipped and full-size frames are allowed twice each (the margin for the larger coordinates of
# the bigger frame).
FIXTURE_EXCESS_PIXELS = 0.00202
FIXTURE_DEVIATION_SPACINGS = 2871.7
DEVIATION_FACTOR = 2.0
MAX_LEFT_OUT = 0.01  # fragments whose interpolated position legitimately differs from the pixel-centre reprojection


def _m(flat):
    return np.array(flat[:], np.float64).reshape(4, 4).T  # column-major flat[16] -> M[row, col]


def reproject(view, depth):
    """(H, W, 2) float64 motion vectors: world position from the pixel centre and `depth` through the fp64 inverses of view->projection and
    view->view, projected with the last-frame matrices, in pixels of view->render_resolution, minus the pixel centre."""
    H, W = depth.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64) + 0.5, np.arange(W, dtype=np.float64) + 0.5, indexing="ij")
    ndc = np.stack([xs / (W * 0.5) - 1.0, ys / (H * 0.5) - 1.0, depth.astype(np.float64), np.ones((H, W))], -1)
    to_world = np.linalg.inv(_m(view.view)) @ np.linalg.inv(_m(view.projection))
    to_last = _m(view.last_frame_projection) @ _m(view.last_frame_view)
    with np.errstate(all="ignore"):
        world = ndc @ to_world.T
        world /= world[..., 3:4]
        last = world @ to_last.T
        uv = last[..., :2] / last[..., 3:4] * 0.5 + 0.5
    res = np.array([view.render_resolution[0], view.render_resolution[1]], np.float64)
    return uv * res - np.stack([xs, ys], -1)


def deviation_in_half_spacings(mv_bits, want, mask):
    """|fp16 value - fp64 reprojection| over the pixels of `mask`, both components, in units of the fp16 spacing at the stored value"""
    got = mv_bits.view(np.float16)
    with np.errstate(all="ignore"):
        dev = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(got)).astype(np.float64)
    return np.where(mask[..., None], dev, 0.0)


def excess_over_store_rounding(mv_bits, want, mask):
    """|fp16 value - fp64 reprojection| minus half a spacing of the fp16 grid at the reprojection (the rounding of the store), not below
    zero, in pixels, over the pixels of `mask`, both components"""
    got = mv_bits.view(np.float16).astype(np.float64)
    with np.errstate(all="ignore"):
        half = 0.5 * np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
        dev = np.maximum(np.abs(got - want) - half, 0.0)
    return np.where(mask[..., None], dev, 0.0)
