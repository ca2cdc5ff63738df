"""VPL extraction and injection (vpl.hip, vpl_inject.hpp) at the boundaries of the machinery that rebuilds the list order: the ballot /
prefix compaction over chunks of 1024 invocations, the 4096-key bitonic sort, the switch to the two-launch form above 4096 lights.
HIP against the oracle's sequential replay, bit for bit (a NaN equals a NaN: tests/list_kernel_cases.py); buffers the kernels must not
write carry sentinels.  The conditions that keep the inputs honest are asserted on the oracle alone in tests/test_list_kernels_cpu.py."""
import numpy as np
import pytest

from tests import list_kernel_cases as L

pytestmark = pytest.mark.gpu


def _extract_and_check(ctx, res, cascade, seed=L.SEED, dark="half", pads=False):
    import torch
    rsm, want, count = L.extraction_case(res, cascade, seed, dark, pads)
    rsm_t = {k: L.to_dev(v) for k, v in rsm.items()}
    list_t, count_t = L.hip_extract(ctx, rsm_t, res, cascade)
    torch.cuda.synchronize()
    what = f"res {res} cascade {cascade} seed {seed} dark {dark}"
    assert int(L.from_dev(count_t, np.uint32)[0]) == count, what
    # the whole buffer: `count` lights in invocation order, the sentinel behind them
    assert np.array_equal(L.from_dev(list_t, np.uint32), want), f"{what}: list buffer differs"
    for k, v in rsm.items():
        assert np.array_equal(L.from_dev(rsm_t[k], v.dtype), v), k
    return list_t, count_t


# res -> invocations: 2 -> 1; 6 -> 9, less than a wave; 62 -> 961, one partial chunk; 66 -> 1089, one full chunk and a 65-entry tail (lanes of
# wave 1 past the end, waves 2..15 empty); 128 -> 4096, the shape of the existing tests; 130 -> 4225, a tail after four chunks and a list longer
# than the sort capacity
@pytest.mark.parametrize("cascade", L.EXTRACT_CASCADES)
@pytest.mark.parametrize("res", L.EXTRACT_RES)
def test_extraction_with_a_sparse_keep_mask(hip_ctx, res, cascade):
    for seed in (L.RES2_SEEDS if res == 2 else (L.SEED,)):
        _extract_and_check(hip_ctx, res, cascade, seed)


@pytest.mark.parametrize("res", (2, 66, 130))
def test_extraction_of_a_dark_rsm_stores_nothing(hip_ctx, res):
    _, want, count = L.extraction_case(res, 0, L.SEED, "all")
    assert count == 0 and (want == L.LIST_SENTINEL).all()
    _extract_and_check(hip_ctx, res, 0, L.SEED, "all")


def test_extraction_with_padded_pitches(hip_ctx):
    """rows three and more texels wider, slices one and more rows taller, differently for flux, normals and depth; the padding is bright"""
    for cascade in L.EXTRACT_CASCADES:
        _extract_and_check(hip_ctx, 66, cascade, pads=True)


def test_extraction_scratch_reuse(hip_ctx):
    """the candidate and keep regions of the context's scratch move with the invocation count: flags of the larger run must not leak"""
    for res in (130, 6, 66, 130, 2):
        _extract_and_check(hip_ctx, res, 3)


def test_full_list_of_4225_goes_straight_into_the_volumes(hip_ctx):
    """nothing dark at res 130: every invocation stores, and the device list feeds sah_lpv_inject_vpls (capacity 4225: two launches)"""
    import torch
    res, cascade = 130, 0
    _, want_list, count = L.extraction_case(res, cascade, L.SEED, "none")
    assert count == 4225
    list_t, count_t = _extract_and_check(hip_ctx, res, cascade, L.SEED, "none")
    start = L.start_volumes(L.SEED + 20)
    want = [v.copy() for v in start]
    L.oracle_inject(np.ascontiguousarray(want_list), count, count, want)
    assert sum(int((w != s).sum()) for w, s in zip(want, start)) > 1000  # light went in
    vols_t = [L.to_dev(v) for v in start]
    L.hip_inject(hip_ctx, list_t, count_t, count, vols_t)
    torch.cuda.synchronize()
    for c in range(3):
        L.assert_same(L.from_dev(vols_t[c], np.uint16), want[c], "f16", f"volume {c}")


# ---- injection -------------------------------------------------------------------------------------------------------------------------------

def _run(ctx, *key):
    case = L.injection_case(*key)
    return L.check_injection_case(ctx, case, " ".join(str(k) for k in key)), case


@pytest.mark.parametrize("count", L.INJECT_COUNTS)
def test_injection_counts_below_the_capacity(hip_ctx, count):
    """capacity 4096 and a buffer full of live lights: only the first `count` go in (wave, row and capacity boundaries)"""
    got, case = _run(hip_ctx, "count", count)
    if count == 0:
        for c in range(3):
            assert np.array_equal(got[c], case["start"][c])


def test_injection_count_word_above_the_capacity(hip_ctx):
    _run(hip_ctx, "overcount")


@pytest.mark.parametrize("count", (4097, 5))
def test_injection_two_launch_form_at_its_smallest(hip_ctx, count):
    _run(hip_ctx, "capacity", 4097, count)


@pytest.mark.parametrize("count", (3000, 4096))
def test_injection_forms_agree(hip_ctx, count):
    """one list through the sorting kernel (capacity 4096) and through the two-launch form (capacity 4097): the same bytes, the oracle's"""
    a, ca = _run(hip_ctx, "capacity", 4096, count)
    b, cb = _run(hip_ctx, "capacity", 4097, count)
    for c in range(3):
        assert np.array_equal(ca["want"][c], cb["want"][c]) and np.array_equal(a[c], b[c])


@pytest.mark.parametrize("capacity", L.FORMS)
@pytest.mark.parametrize("kind", L.PILE_KINDS)
def test_injection_piles(hip_ctx, kind, capacity):
    """4096 lights in one cell (or two, alternating): the longest serial run, where list order and the rounding after every addition decide"""
    _run(hip_ctx, "pile", kind, capacity)


@pytest.mark.parametrize("capacity", L.FORMS)
def test_injection_of_dropped_lights_changes_nothing(hip_ctx, capacity):
    got, case = _run(hip_ctx, "dropped", capacity)
    for c in range(3):
        assert np.array_equal(got[c], case["start"][c])


@pytest.mark.parametrize("capacity", L.FORMS)
@pytest.mark.parametrize("which", (0, 1))
def test_injection_extents_cascades_and_pitches(hip_ctx, which, capacity):
    """64 x 32 x 32 with two cascades (cascade 1) and 40 x 36 x 33 with one; the three channel volumes have different, poisoned padding"""
    _run(hip_ctx, "extent", which, capacity)


@pytest.mark.parametrize("capacity", L.FORMS)
@pytest.mark.parametrize("family", ("finite", "family_b"))
def test_injection_of_colours_that_make_nan(hip_ctx, family, capacity):
    """zero normals (NaN coefficients) and, for family (b), every colour bit pattern: a NaN must be a NaN, a number the same number"""
    _run(hip_ctx, family, capacity)
