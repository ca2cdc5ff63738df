"""Memory layouts for every entry point, not only Lighting: images described by hand with a row pitch (and slice pitch) larger than the
payload and a shifted base, built on tests.lighting_cases.Pitched.  A test runs an entry point on the same logical inputs once tightly packed
and once (or more) padded, and asserts three things:

  1. the padded run meets the oracle by the bar of the entry point's tight test,
  2. the padded run equals the tight run bit for bit (a result must not depend on where its images lie),
  3. no byte of padding changed, in inputs and outputs alike, and every input still holds what was uploaded.

A `spec` maps the name of an image to dict(row_pad=, offset=, slice_pad=) in bytes; an image without an entry is tight (still wrapped, so that
the tests handle one kind of object).  The two families of specs the tests use:
  A  the smallest row padding and base offset the entry point's argument check admits (8 bytes for RGBA16F, 4 for 32-bit texels, 2 for D16, 1
     byte of row padding for R8 with a base that stays 4-byte aligned),
  B  a padding that is a multiple of the texel size but not of 16, and for volumes a slice padding that is not a multiple of the row pitch."""
import numpy as np

from androidrenderer_amd import _abi
from tests.lighting_cases import SENTINEL, Pitched  # noqa: F401  (re-exported)

NAN_FILL = 0xFF  # every half (0xFFFF) and every float (0xFFFFFFFF) of the padding is a NaN

RGBA16F = _abi.FORMAT_R16G16B16A16_SFLOAT
RGBA8 = _abi.FORMAT_R8G8B8A8_UNORM
SRGBA8 = _abi.FORMAT_R8G8B8A8_SRGB
R32F = _abi.FORMAT_R32_SFLOAT
D32F = _abi.FORMAT_D32_SFLOAT
D16 = _abi.FORMAT_D16_UNORM
R8 = _abi.FORMAT_R8_UNORM
RG16F = _abi.FORMAT_R16G16_SFLOAT
R11G11B10 = _abi.FORMAT_B10G11R11_UFLOAT_PACK32


def pitched(a, fmt, dims, spec=None, fill=SENTINEL):
    return Pitched(a, fmt, dims, fill=fill, **(spec or {}))


def wrap(arrays, formats, spec=None, fill=SENTINEL):
    """{key: array} -> {key: Pitched} for the keys of `formats` ({key: (format, 2 | 3)}), numpy and torch alike; other keys pass through."""
    spec = spec or {}
    assert set(spec) <= set(formats), f"layout for unknown images: {set(spec) - set(formats)}"
    return {k: pitched(v, formats[k][0], formats[k][1], spec.get(k), fill) if k in formats else v for k, v in arrays.items()}


def _images(wrapped):
    if isinstance(wrapped, Pitched):
        return [("image", wrapped)]
    if isinstance(wrapped, dict):
        return [(k, v) for k, v in wrapped.items() if isinstance(v, Pitched)]
    return [(str(i), v) for i, v in enumerate(wrapped) if isinstance(v, Pitched)]


def assert_padding_intact(*groups, what=""):
    """every wrapped image of every group (a Pitched, a dict or a list of them): no byte outside the payload differs from its fill value"""
    for g in groups:
        for k, p in _images(g):
            assert p.padding_intact(), f"{what}: the padding of '{k}' (row pitch {p.row_pitch}, offset {p.offset}) was written"


def assert_inputs_unchanged(*groups, what=""):
    """every wrapped image still holds, bit for bit, the array it was made from (for images a call only reads)"""
    for g in groups:
        for k, p in _images(g):
            want = p.logical if p.is_np else p.logical.contiguous().cpu().numpy()
            got = p.read(want.dtype)
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), f"{what}: input '{k}' changed"


def assert_rows_untouched(before, after, row_begin, row_end, what=""):
    """rows of an output outside [row_begin, row_end) hold what they held before the call (`before`, `after`: arrays with the row axis first;
    `before` may be a scalar payload)"""
    before = np.broadcast_to(before, after.shape)
    keep = np.ones(before.shape[0], bool)
    keep[row_begin:row_end] = False
    assert np.array_equal(before[keep], after[keep]), f"{what}: rows outside [{row_begin}, {row_end}) were written"


def padded_columns(a, pad, fill=SENTINEL):
    """`a` (H, W[, C]), numpy or torch, as a column slice of a wider array whose `pad` extra columns hold `fill` bytes: same values, a row
    stride larger than the payload, the texel stride unchanged — how a texture level with padded rows reaches mesh.geometry().
    Returns (the slice, the wide array)."""
    w = a.shape[1]
    if isinstance(a, np.ndarray):
        wide = np.empty((a.shape[0], w + pad) + a.shape[2:], a.dtype)
        wide.view(np.uint8)[...] = fill
    else:
        import torch
        assert a.dtype == torch.uint8
        wide = torch.full((a.shape[0], w + pad) + tuple(a.shape[2:]), fill, dtype=a.dtype, device=a.device)
    wide[:, :w] = a
    return wide[:, :w], wide


def pad_texture_levels(textures, fill=SENTINEL):
    """the `textures` entry of mesh.Mesh.arrays() / mesh.to_device() with every level given padded rows: 1, 2 or 3 extra texels, a different
    number on neighbouring levels.  Returns (textures, [(wide array, payload width)])."""
    out, wides = [], []
    n = 0
    for mips, fmt, smp in textures:
        levels = []
        for m in mips:
            view, wide = padded_columns(m, 1 + n % 3, fill)
            n += 1
            levels.append(view)
            wides.append((wide, m.shape[1]))
        out.append((levels, fmt, smp))
    return out, wides


def assert_texture_padding_intact(wides, fill=SENTINEL):
    for wide, w in wides:
        assert bool((wide[:, w:] == fill).all()), "the padding of a texture level was written"
