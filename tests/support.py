"""What the tests of the screen-space passes share: device planes with guard bytes, the byte comparison and its message, malformed copies of a
plane, the context's state, a context on a side stream, the ViewData of a restatement's view, and the run of a fuzz child.  A plain module:
the test of a new pass imports from here (and tests/host_programs.py for its C++ program) and copies nothing from its predecessor."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from androidrenderer_amd import _abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


class Image:
    """A device plane of `bpp`-byte texels with a pitch of its own; bytes that belong to no texel hold SENTINEL."""

    def __init__(self, fmt, w, h, pitch=None, data=None, offset=0):
        import torch
        self.bpp = _abi.FORMAT_BPP[fmt]
        self.w, self.h, self.pitch, self.offset = w, h, (w * self.bpp if pitch is None else pitch), offset
        host = np.full(self.offset + self.h * self.pitch + 64, SENTINEL, np.uint8)
        if data is not None:
            rows = np.ascontiguousarray(data).view(np.uint8).reshape(h, w * self.bpp)
            host[self.offset:self.offset + h * self.pitch].reshape(h, self.pitch)[:, :w * self.bpp] = rows
        self.host_in = host.copy()
        self.t = torch.from_numpy(host).cuda()
        self.plane = _abi.Plane(self.t.data_ptr() + self.offset, w, h, self.pitch, fmt)

    def bytes(self):
        return self.t.cpu().numpy()

    def texels(self, dtype):
        b = self.bytes()[self.offset:self.offset + self.h * self.pitch].reshape(self.h, self.pitch)[:, :self.w * self.bpp]
        return np.ascontiguousarray(b).view(dtype)

    def padding_intact(self, rows=None):
        """no byte outside the texels (of `rows`, default all) changed"""
        b = self.bytes()
        mask = np.ones(b.shape, bool)
        body = mask[self.offset:self.offset + self.h * self.pitch].reshape(self.h, self.pitch)
        r0, r1 = rows if rows is not None else (0, self.h)
        body[r0:r1, :self.w * self.bpp] = False
        return bool((b[mask] == self.host_in[mask]).all())

    def unchanged(self):
        return bool((self.bytes() == self.host_in).all())


# ---- comparing ------------------------------------------------------------------------------------------------------------------------------
def _raw(a):
    return a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()


def same(got, want):
    """bit for bit: the bytes of the two arrays (or bytes objects) are equal — a NaN equals itself, -0 is not +0"""
    return _raw(got) == _raw(want)


def differs(got, want):
    """the message for a failed same() of two arrays (y, x[, channels]): compared per texel as bytes, so it agrees with same()"""
    as_bytes = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[:2] + (-1,))  # noqa: E731
    bad = (as_bytes(got) != as_bytes(want)).any(-1)
    return f"{int(bad.sum())} of {bad.size} texels differ, first (y, x) at {np.argwhere(bad)[:4].tolist()}"


# ---- malformed copies of a plane, for the refusal tests -----------------------------------------------------------------------------------------
def retyped(plane, fmt):
    """a copy of the _abi.Plane (or _abi.Volume) with another format"""
    return type(plane)(*[getattr(plane, n) for n, _ in plane._fields_[:-1]], fmt)


def resized(plane, width, height):
    """a copy of the _abi.Plane with another extent over the same memory and pitch"""
    return _abi.Plane(plane.ptr, width, height, plane.row_pitch_bytes, plane.format)


# ---- contexts -------------------------------------------------------------------------------------------------------------------------------
def context_state(ctx):
    """what a pass with no side effects on the context leaves as it was"""
    return ctx.cache_epoch(), ctx.lighting_dispatch(), ctx.copy_rebuilds()


@contextlib.contextmanager
def side_stream_context():
    """(ctx, stream): a context of its own on a side stream of its own; on the way out the device is synchronised and the context closed"""
    import torch
    stream = torch.cuda.Stream()
    ctx = lib.Context(0)
    try:
        ctx.set_stream(stream.cuda_stream)
        yield ctx, stream
    finally:
        torch.cuda.synchronize()
        ctx.close()


def hip_runtime():
    """the HIP runtime this process already uses (the one the stream and the library live in)"""
    paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(paths) == 1, paths
    return C.CDLL(paths[0])


# ---- the ViewData of a restatement's view --------------------------------------------------------------------------------------------------------
def _view_data(view, matrices):
    v = _abi.ViewData()
    for name in matrices:
        for i in range(16):
            getattr(v, name)[i] = float(getattr(view, name)[i])
    v.projection[0], v.projection[5], v.projection[8], v.projection[9], v.z_near = float(view.p00), float(view.p11), float(view.p20), float(view.p21), float(view.z_near)
    v.projection[11] = -1.0
    return v


def view_data_of(view):
    """an _abi.ViewData holding what a pass of one frame reads (ssao, ssr), from the restatement's View: the view matrix and the projection"""
    return _view_data(view, ("view",))


def reprojection_view_data_of(view):
    """an _abi.ViewData holding what a reprojecting pass reads (the two denoisers), from the restatement's View: inverse_view, last_frame_view
    and the projection"""
    return _view_data(view, ("inverse_view", "last_frame_view"))


# ---- fuzz children ----------------------------------------------------------------------------------------------------------------------------
def run_fuzz_child(script, seed, iterations, timeout=600, tail_lines=10):
    """tests/<script> SEED ITERATIONS in a child process, so that a fault inside the library is a failed test: skips where the child says
    SKIP: (a HIP device is present), asserts that it ended with 0 and its OK: line, returns its output for what the test checks on top."""
    import pytest
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), str(seed), str(iterations)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=timeout)
    tail = "\n".join(r.stdout.splitlines()[-tail_lines:])
    if "SKIP:" in r.stdout:
        pytest.skip(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0, f"the fuzz child ended with code {r.returncode} (negative: a signal — a fault inside the library):\n{tail}"
    assert f"OK: {iterations} iterations" in r.stdout, tail
    return r.stdout
