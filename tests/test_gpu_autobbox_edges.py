"""The minimum filter, the min / max reduction and the box of csrc/autobbox.hip and
csrc/minmax.hpp at their edges -- the seams of both tile classes along every axis, every
level count and the extremes of the overlap shift, the ragged last tile in every residue of
the 4-wide loop, special values across a seam, the reduction's block, round and tail, a
filtered value on the threshold, a NaN against it, and calls over stale workspace buffers --
bit for bit against tests/autobbox_ref.py (floats through their uint32 view).  The cases are
tests/autobbox_cases.py's; what they rely on is proved in tests/test_autobbox_premises_cpu.py.

Where each branch of the kernels runs (shapes (nz, ny, nx)):
  k_minfilter<0>, nat > 1, both classes      test_radius_sweep[x-*], test_length_sweep[x-*]: 65 rows
  k_minfilter<1>, <2, false>, nat > 1        the same with y-*, z-*: nx = 66, two line groups
  tile 64 / 128 on both sides of r = 16 / 17 r16, r17 of the sweeps; test_random_volumes (70, 45, 130)
  1 .. 7 levels, shift 1 and p - 1           test_radius_sweep: r = 2^j and 2^j - 1
  the remainder of the 4-wide loop           test_length_sweep (full tiles), test_positive_ragged_tile
  the zero extension at large radii          test_random_volumes
  NaN, +-0, -Inf over a seam; +Inf           test_special_values_across_a_seam, test_infinite_image
  k_minmax_partial / _final with BoxMinMax   test_min_max_*: one thread .. the third round's tail
  k_threshold_box beyond one round           test_six_faces
  k_minfilter<2, true>, found = 1, tile 128  test_fused_pass_in_the_large_class
  double(v) > thr in both kernels            test_value_on_the_threshold, test_nan_against_the_threshold
  the grow-only workspace                    test_calls_do_not_depend_on_the_calls_before
"""
import numpy as np
import pytest
import torch

import autobbox_cases as ac
import autobbox_ref as ar
from spim_registration_amd import boundingbox as bb

pytestmark = pytest.mark.gpu


def u32(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return ac.u32(a)


def on_device(img):
    return torch.from_numpy(np.array(img, np.float32)).cuda()      # (a copy: the cases are read-only)


def check_filter(img, r, want, host=False):
    got = bb.min_filter(img if host else on_device(img), r)
    assert tuple(got.shape) == img.shape
    np.testing.assert_array_equal(u32(got), u32(want))


def box_of(res):
    return [list(res[0]), list(res[1]), res[2]]


def check_segment(img, background, r, want=None):
    """segment_bounds from a device image, with and without the filtered image, against ar.segment"""
    want = ar.segment(img, background, r) if want is None else want
    dimg = on_device(img)
    for filtered in (False, True):
        got = bb.segment_bounds(dimg, background, r, return_filtered=filtered)
        np.testing.assert_array_equal(u32((got["min"], got["max"])), u32((want["min"], want["max"])))
        np.testing.assert_array_equal(np.float64(got["threshold"]).view(np.uint64),
                                      np.float64(want["threshold"]).view(np.uint64))
        assert (list(got["bounds_min"]), list(got["bounds_max"]), got["found"]) == (
            want["bounds_min"], want["bounds_max"], want["found"])
        if filtered:
            np.testing.assert_array_equal(u32(got["filtered"]), u32(want["filtered"]))
    return want


def test_tile_sizes_are_the_ones_the_cases_straddle(gpu):
    """The constants the cases of tests/autobbox_cases.py are built around, as the library
    reports them (csrc/autobbox.hip: kMfLines, kMfTileSmall, kMfTileLarge, kMfSmallRadius;
    csrc/minmax.hpp: kRedBlock, kRedGrid).  Whoever changes the tiling moves the seams: revisit
    the sweeps, the special values and the reduction lengths."""
    assert bb.min_filter_tiles() == (ac.LINES, ac.TILE_SMALL, ac.TILE_LARGE, ac.SMALL_RADIUS, ac.RED_BLOCK,
                                     ac.RED_GRID)
    assert bb.min_filter_tiles() == (64, 64, 128, 16, 256, 1024) and ac.ROUND == 1024 * 256


# ------------------------------------------------------------------ the filter
@pytest.mark.parametrize("name", [c.name for c in ac.RADIUS_SWEEP])
def test_radius_sweep(gpu, name):
    """every radius at which the tile, the level count or the shift changes, once per pass axis:
    three tiles, the last of 3 outputs, on an additive image"""
    check_filter(ac.sweep_image(name), ac.SWEEPS[name].r, ac.sweep_expected(name))


@pytest.mark.parametrize("name", [c.name for c in ac.LENGTH_SWEEP])
def test_length_sweep(gpu, name):
    """one short of a tile, a tile, 1, 2 and 3 past it, two tiles and one past, per axis and class"""
    check_filter(ac.sweep_image(name), ac.SWEEPS[name].r, ac.sweep_expected(name))


@pytest.mark.parametrize("name", ["x-r3-n67", "y-r17-n131"])
def test_sweep_case_from_a_host_array(gpu, name):
    check_filter(ac.sweep_image(name), ac.SWEEPS[name].r, ac.sweep_expected(name), host=True)


@pytest.mark.parametrize("name", list(ac.POSITIVES))
def test_positive_ragged_tile(gpu, name):
    """a positive image: the zero extension decides the outputs of the ragged last tile"""
    c = ac.POSITIVES[name]
    img = ac.positive_image(name)
    check_filter(img, c.r, ar.min_filter(img, c.r))


@pytest.mark.parametrize("shape,r", ac.RANDOM_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"r{v}")
def test_random_volumes(gpu, shape, r):
    """[-1, 1] with more than one large tile along x and along z; (70, 45, 130) on both sides of
    the switch between the tiles"""
    img = ac.random_volume(shape)
    check_filter(img, r, ar.min_filter(img, r))


@pytest.mark.parametrize("name", list(ac.SPECIALS))
def test_special_values_across_a_seam(gpu, name):
    """one NaN whose footprint straddles the first seam of every axis, +0 / -0 on the two sides of
    an x seam, one -Inf, in both tile classes"""
    img = ac.special_image(name)
    r = ac.SPECIALS[name].r
    want = ar.min_filter(img, r)
    check_filter(img, r, want)
    check_filter(img, r, want, host=True)


@pytest.mark.parametrize("name", list(ac.INF_CASES))
def test_infinite_image(gpu, name):
    """all +Inf: Float.MAX_VALUE inside, the zero extension's 0 within r of a face"""
    shape, r = ac.INF_CASES[name]
    img = ac.inf_image(name)
    want = ar.min_filter(img, r)
    assert want[shape[0] // 2, shape[1] // 2, shape[2] // 2] == ar.FLOAT_MAX and want[0, 0, 0] == 0
    check_filter(img, r, want)


# ------------------------------------------------------------------ min / max
def check_min_max(flat, shape):
    want = ac.minmax_ref(flat)
    got = bb.min_max(on_device(flat.reshape(shape)))
    np.testing.assert_array_equal(u32(got), u32(want), err_msg=str(shape))
    return got


@pytest.mark.parametrize("n", ac.MINMAX_LENGTHS)
def test_min_max_planted_extrema(gpu, n):
    """a constant 0.5 with a single -1 and, separately, a single 2 at a wave's, a block's and a
    round's last and first element and at the end, as dims (n, 1, 1) and in a factorisation"""
    for shape in ac.minmax_shapes(n):
        for at in ac.plant_indices(n):
            assert check_min_max(ac.planted(n, at, -1.0), shape)[0] == -1.0
            assert check_min_max(ac.planted(n, at, 2.0), shape)[1] == 2.0


@pytest.mark.parametrize("n", ac.MINMAX_LENGTHS)
def test_min_max_special_values(gpu, n):
    """a NaN, a -0 among +0 and a +0 among -0 as the last element; all +Inf and all -Inf"""
    sp = ac.minmax_specials(n)
    shape = ac.minmax_shapes(n)[-1]
    assert all(np.isnan(v) for v in check_min_max(sp["nan_last"], shape))
    got = check_min_max(sp["negative_zero_last"], shape), check_min_max(sp["positive_zero_last"], shape)
    if n > 1:          # (one voxel: the image holds one of the zeros only)
        assert u32(got[0]).tolist() == u32(got[1]).tolist() == [0x80000000, 0]
    assert check_min_max(sp["all_pinf"], shape) == (ar.FLOAT_MAX, np.inf)
    assert check_min_max(sp["all_ninf"], shape) == (-np.inf, -ar.FLOAT_MAX)


# ------------------------------------------------------------------ the box
def test_six_faces(gpu):
    """beyond one round of k_threshold_box's grid stride, six voxels each alone on one face"""
    img = ac.faces_image()
    want = ar.threshold_bounds(img, ac.FACES_THRESHOLD)
    assert box_of(bb.threshold_bounds(on_device(img), ac.FACES_THRESHOLD)) == list(want)
    for name in ac.FACES:
        img = ac.faces_image(without=name)
        assert box_of(bb.threshold_bounds(on_device(img), ac.FACES_THRESHOLD)) == list(
            ar.threshold_bounds(img, ac.FACES_THRESHOLD)), name


def test_fused_pass_in_the_large_class(gpu):
    """r = 17 with found = 1: the six faces are decided in both z tiles and both x line groups"""
    want = check_segment(ac.fused_image(), ac.FUSED_BACKGROUND, ac.FUSED_RADIUS)
    assert want["found"] and (want["bounds_min"], want["bounds_max"]) == ac.FUSED_BOX
    thr = want["threshold"]
    assert box_of(bb.threshold_bounds(on_device(want["filtered"]), thr)) == [*ac.FUSED_BOX, True]


@pytest.mark.parametrize("r", list(ac.EXACT))
def test_value_on_the_threshold(gpu, r):
    """filtered values exactly 0.5 = the threshold stay out, nextafter(0.5, 1) makes the box:
    in the fused z pass and in k_threshold_box"""
    img = ac.exact_image(r)
    want = check_segment(img, ac.EXACT_BACKGROUND, r)
    assert want["threshold"] == 0.5 and (want["bounds_min"], want["bounds_max"]) == ac.EXACT[r][3]
    assert box_of(bb.threshold_bounds(on_device(want["filtered"]), 0.5)) == [*ac.EXACT[r][3], True]


def test_nan_against_the_threshold(gpu):
    """a NaN is not above a threshold, and nothing is above a NaN threshold"""
    clean, dirty = ac.nan_images()
    thr = ar.segment(clean, ac.NAN_BACKGROUND, ac.NAN_RADIUS)["threshold"]
    want = check_segment(dirty, ac.NAN_BACKGROUND, ac.NAN_RADIUS)          # the threshold is NaN
    assert not want["found"] and want["bounds_max"] == [0, 0, 0]
    assert box_of(bb.threshold_bounds(on_device(want["filtered"]), thr)) == [*ac.NAN_BOX, True]
    assert box_of(bb.threshold_bounds(on_device(want["filtered"]), thr)) == list(
        ar.threshold_bounds(want["filtered"], thr))


# ------------------------------------------------------------------ the workspace
def test_calls_do_not_depend_on_the_calls_before(gpu):
    """One process, one device, this order: a large filter call (every buffer grows), a
    segmentation of a smaller image with found = 1 (over stale tails in t1 and t2), min / max of
    one voxel (over stale partials in red), a box with nothing found right after a found one,
    release_workspace, and the first call again.  Each result is its restatement."""
    big = ac.random_volume((140, 9, 131))
    big_want = ar.min_filter(big, 33)
    check_filter(big, 33, big_want, host=True)                              # host: staged through t2, out through t1
    np.testing.assert_array_equal(u32(bb.min_max(big)), u32(ar.min_max_fast(big)))     # 645 partials in red
    clean, _ = ac.nan_images()
    want = check_segment(np.ascontiguousarray(clean), ac.NAN_BACKGROUND, ac.NAN_RADIUS)
    assert want["found"] and (want["bounds_min"], want["bounds_max"]) == ac.NAN_BOX
    host = bb.segment_bounds(clean, ac.NAN_BACKGROUND, ac.NAN_RADIUS, return_filtered=True)
    np.testing.assert_array_equal(u32(host["filtered"]), u32(want["filtered"]))
    assert (list(host["bounds_min"]), list(host["bounds_max"]), host["found"]) == (*ac.NAN_BOX, True)
    one = np.full((1, 1, 1), 0.25, np.float32)
    np.testing.assert_array_equal(u32(bb.min_max(one)), u32(ar.min_max(one)))
    empty = np.zeros(ac.NAN_SHAPE, np.float32)
    assert bb.threshold_bounds(empty, 0.5) == (ac.NAN_SHAPE[::-1], (0, 0, 0), False)
    bb.release_workspace(0)
    check_filter(big, 33, big_want, host=True)
