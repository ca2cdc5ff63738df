"""CPU companion of tests/test_pos_div_shared_gpu.py: which cameras of tests/lighting_cases.py meet the host's half of the condition for the
shared-reciprocal divide under zeros of either sign (api.cpp: detect_fast_path, FastArgs::pos_div_shared — restated here from DESIGN.md §5a, not
from api.cpp's result), and where the column / row table holds a -0 numerator, which is the device's half."""
import math

import numpy as np
import pytest

from tests import lighting_cases as lc
from tests.test_pos_div_shared_gpu import _negate_p0, _table_has_neg_zero


def _host_condition(view, width, height):
    """(pos_div_nr, pos_div_shared before the table is consulted)"""
    P = list(view.gpu_data.inverse_projection)
    r = view.gpu_data.render_resolution
    bounded = (P[10] == 0.0 and P[12] == 0.0 and P[13] == 0.0 and 2.0 ** -16 <= abs(P[0]) <= 2.0 ** 30 and 2.0 ** -16 <= abs(P[5]) <= 2.0 ** 30
               and 2.0 ** -40 <= abs(P[14]) <= 2.0 ** 40 and r[0] > 0 and r[1] > 0 and width <= 256.0 * r[0] and height <= 256.0 * r[1])
    plus = all(math.copysign(1.0, P[i]) == 1.0 for i in (12, 13))
    return int(bounded and plus), int(bounded and not plus)


# camera -> (pos_div_nr, host half of pos_div_shared): jitter puts numbers into [12], [13]; every other camera keeps make_view's -0.0
WANT = {"default": (0, 1), "plus_zero": (1, 0), "jitter": (0, 0), "yaw37": (0, 1), "down": (0, 1), "up": (0, 1), "far": (0, 1), "fov5": (0, 1),
        "halfres": (0, 1)}


@pytest.mark.parametrize("cam", sorted(lc.CAMERAS))
def test_which_cameras_meet_the_host_condition(cam):
    view = lc.make_view(256, 144, **dict(lc.DEFAULT_CAMERA, **lc.CAMERAS[cam]))
    assert _host_condition(view, 256, 144) == WANT[cam]


@pytest.mark.parametrize("edit,want", [("ortho", (0, 0)), ("p0_tiny", (0, 0)), ("plus_zero", (1, 0))])
def test_the_kept_cameras_stay_where_they_were(edit, want):
    """[10] != 0 and |p0| < 2^-16 fail the bounds whatever the signs; so does a render resolution below width / 256"""
    assert _host_condition(lc.make_view(192, 108, edit=edit), 192, 108) == want
    assert _host_condition(lc.make_view(256, 144, res_scale=1.0 / 300.0), 256, 144) == (0, 0)


def test_every_matrix_case_keeps_its_pos_div_nr():
    """the new condition is disjoint from pos_div_nr: a case of the matrix that expects pos_div_nr == 1 never meets it"""
    for case in lc.CASES:
        if case.expect.get("family") != "fast" and case.expect.get("tiled_fast_geom") != 1:
            continue
        cam = dict(lc.DEFAULT_CAMERA, **(case.frame.get("camera") or {}))
        nr, shared = _host_condition(lc.make_view(case.width, case.height, **cam), case.width, case.height)
        assert nr == case.expect.get("pos_div_nr", 0) and not (nr and shared), case.name


def test_tables_of_the_default_camera_hold_no_neg_zero_and_a_mirrored_one_does():
    class F:
        pass
    for w, h in ((256, 144), (192, 96), (3840, 2160), (131, 37)):
        f = F()
        f.width, f.height, f.view = w, h, lc.make_view(w, h)
        assert not _table_has_neg_zero(f), (w, h)
        _negate_p0(f)
        # the GLSL texcoord (x + 1) / W is 0.5 at an even W's centre column, the Slang one (x + 0.5) / W at an odd W's: ndc.x == +0 either way
        assert _table_has_neg_zero(f), (w, h)
