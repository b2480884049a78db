"""CPU: the restatement of the reference's automatic bounding box (tests/autobbox_ref.py)
against known answers, a brute-force window minimum, and the premise of the end-to-end GPU test."""
import numpy as np
import pytest

import autobbox_ref as ar


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def brute_min_filter(img, r):
    """The 3-D window minimum over the zero extension, one window at a time."""
    nz, ny, nx = img.shape
    ext = np.pad(img, r, constant_values=np.float32(0.0))
    out = np.empty_like(img)
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                out[z, y, x] = min(ext[z:z + 2 * r + 1, y:y + 2 * r + 1, x:x + 2 * r + 1].min(), ar.FLOAT_MAX)
    return out


def test_java_min_max_semantics():
    nan, nz, pz = np.float32(np.nan), np.float32(-0.0), np.float32(0.0)
    assert np.isnan(ar.jmin(nan, 1.0)) and np.isnan(ar.jmin(1.0, nan))
    assert np.isnan(ar.jmax(nan, 1.0)) and np.isnan(ar.jmax(1.0, nan))
    assert np.signbit(ar.jmin(pz, nz)) and np.signbit(ar.jmin(nz, pz))
    assert not np.signbit(ar.jmax(pz, nz)) and not np.signbit(ar.jmax(nz, pz))
    assert ar.jmin(2.0, -3.0) == -3 and ar.jmax(2.0, -3.0) == 2
    # both start values survive an image of infinities
    inf = np.full((2, 2, 2), np.inf, np.float32)
    assert ar.min_max(inf) == (ar.FLOAT_MAX, np.float32(np.inf))
    assert ar.min_max(-inf) == (np.float32(-np.inf), -ar.FLOAT_MAX)
    a = np.float32([[[3, -0.0, 0.0, 7]]])
    mn, mx = ar.min_max(a)
    assert mn == 0 and np.signbit(mn) and mx == 7
    a[0, 0, 3] = np.nan
    assert all(np.isnan(v) for v in ar.min_max(a))
    rng = np.random.default_rng(1)
    b = (rng.random((3, 5, 7)) * 2 - 1).astype(np.float32)
    b[1, 2, 3] = -0.0
    for img in (a, b, np.zeros((1, 1, 1), np.float32)):
        np.testing.assert_array_equal(u32(ar.min_max_fast(img)), u32(ar.min_max(img)))


def test_threshold_arithmetic():
    mn, mx = np.float32(0.1), np.float32(0.7)
    assert ar.threshold(mn, mx, 5.0) == float(np.float64(np.float32(mx - mn)) * 0.05 + np.float64(mn))
    # the difference is rounded to float before anything happens in double
    mn, mx = np.float32(1e-8), np.float32(1.0)
    assert np.float32(mx - mn) == np.float32(1.0)
    assert ar.threshold(mn, mx, 50.0) == 0.5 + float(np.float64(mn))


@pytest.mark.parametrize("s,r", [(7, 1), (7, 2), (7, 3), (6, 3), (5, 2), (4, 2), (1, 1)])
def test_cube_erodes_to_s_minus_2r(s, r):
    img = np.zeros((15, 16, 17), np.float32)
    img[4:4 + s, 5:5 + s, 6:6 + s] = 2.0
    out = ar.min_filter(img, r)
    want = np.zeros_like(img)
    t = s - 2 * r
    if t > 0:
        want[4 + r:4 + r + t, 5 + r:5 + r + t, 6 + r:6 + r + t] = 2.0
    else:
        assert s < 2 * r + 1
    np.testing.assert_array_equal(out, want)


def test_zero_extension_erodes_from_outside():
    img = np.zeros((9, 9, 9), np.float32)
    img[0:5, 2:7, 2:7] = 1.0          # touches the z = 0 face
    out = ar.min_filter(img, 1)
    want = np.zeros_like(img)
    want[1:4, 3:6, 3:6] = 1.0         # eroded at z = 0 as well: the extension is 0
    np.testing.assert_array_equal(out, want)
    # an image above 0 everywhere loses its outer shell
    out = ar.min_filter(np.full((5, 6, 7), 3.0, np.float32), 2)
    want = np.zeros((5, 6, 7), np.float32)
    want[2:3, 2:4, 2:5] = 3.0
    np.testing.assert_array_equal(out, want)


def test_negative_image_is_not_eroded_at_the_faces():
    img = np.full((4, 5, 6), -5.0, np.float32)
    np.testing.assert_array_equal(ar.min_filter(img, 2), img)      # min(-5, 0) = -5
    img[1, 2, 3] = -7.0
    out = ar.min_filter(img, 1)
    want = img.copy()
    want[0:3, 1:4, 2:5] = -7.0
    np.testing.assert_array_equal(out, want)


@pytest.mark.parametrize("shape,r", [((6, 7, 8), 1), ((6, 7, 8), 2), ((2, 9, 3), 3), ((3, 1, 11), 5), ((1, 1, 1), 1)])
def test_filter_against_brute_force(shape, r):
    """also with axes shorter than the window"""
    rng = np.random.default_rng(shape[2] * 10 + r)
    img = (rng.random(shape) * 2 - 1).astype(np.float32)
    np.testing.assert_array_equal(u32(ar.min_filter(img, r)), u32(brute_min_filter(img, r)))


def test_filter_nan_and_signed_zero():
    img = np.ones((3, 5, 9), np.float32)
    img[1, 2, 4] = np.nan
    out = ar.min_filter(img, 1)
    assert np.isnan(out[0:3, 1:4, 3:6]).all() and np.isnan(out).sum() == 27      # spreads through the window
    img = np.ones((1, 1, 9), np.float32)
    img[0, 0, 3] = 0.0
    img[0, 0, 4] = -0.0
    out = ar.min_filter_axis(img, 1, 2)
    # the window of x = 2 holds +0 only; those of 3, 4, 5 hold -0, which wins; the ends meet the extension's +0
    assert out[0, 0, 2] == 0 and not np.signbit(out[0, 0, 2])
    assert np.signbit(out[0, 0, 3:6]).all() and (out[0, 0, 3:6] == 0).all()
    assert not np.signbit(out[0, 0, 0]) and out[0, 0, 0] == 0 and out[0, 0, 6] == 1


def test_rounding_and_integer_divisions():
    assert [ar.java_round(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, -2.51, 2.49)] == [1, 2, 3, 0, -1, -2, -3, 2]
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    m = ident.copy()
    m[:, 3] = (-2.5, 0.5, 10.49)
    # corners 0 .. 9, 0 .. 19, 0 .. 29, shifted: min -2.5 -> -2, max 6.5 -> 7; 0.5 -> 1, 19.5 -> 20; 10.49 -> 10, 39.49 -> 39
    assert ar.max_bounding_box([(10, 20, 30)], [m], 4) == ([-2, 1, 10], [7, 20, 39], [10, 20, 30], [2, 5, 7])
    # two views; a flip makes the far corner the minimum
    f = ident.copy()
    f[0, 0] = -1.0
    f[0, 3] = 4.0
    assert ar.max_bounding_box([(10, 20, 30), (8, 3, 3)], [ident, f], 3) == (
        [-3, 0, 0], [9, 19, 29], [13, 20, 30], [4, 6, 10])
    assert ar.radii(25, 4) == (12, 3) and ar.radii(5, 4) == (2, 1) and ar.radii(1, 1) == (0, 1)
    assert ar.radii(100, 1) == (50, 50) and ar.radii(9, 2) == (4, 2)


def test_threshold_bounds():
    img = np.zeros((4, 5, 6), np.float32)
    assert ar.threshold_bounds(img, 0.0) == ([6, 5, 4], [0, 0, 0], False)      # the inverted box, as the reference
    img[3, 4, 5] = 1.0
    assert ar.threshold_bounds(img, 0.5) == ([5, 4, 3], [5, 4, 3], True)
    img[0, 0, 0] = 1.0
    assert ar.threshold_bounds(img, 0.5) == ([0, 0, 0], [5, 4, 3], True)
    assert ar.threshold_bounds(img, 1.0) == ([6, 5, 4], [0, 0, 0], False)      # > in double: equal does not count
    v = np.float32(0.3)
    up = np.nextafter(v, np.float32(1))
    img[:] = v
    img[1, 2, 3] = up
    between = (float(v) + float(up)) / 2
    assert ar.threshold_bounds(img, between) == ([3, 2, 1], [3, 2, 1], True)
    img[2, 2, 2] = np.nan
    assert ar.threshold_bounds(img, between) == ([3, 2, 1], [3, 2, 1], True)


def test_auto_bounding_box_scales_back_and_pads():
    fused = np.zeros((10, 12, 14), np.float32)
    fused[2:9, 3:10, 4:12] = 1.0
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    ident[:, 3] = (-7, 3, 0)
    views = [np.zeros((41, 49, 57), np.float32)]         # maximal box min (-7, 3, 0), dims (57, 49, 41): fused (14, 12, 10)
    res = ar.auto_bounding_box(views, [ident], 5.0, 9, 4, fused=fused)
    assert (res["radius_min"], res["eff_radius"], res["fused_dims"]) == (4, 1, [14, 12, 10])
    assert res["threshold"] == 0.05 and res["found"]
    assert (res["bounds_min"], res["bounds_max"]) == ([5, 4, 3], [10, 8, 7])
    assert res["bb_min"] == [5 * 4 - 7 - 12, 4 * 4 + 3 - 12, 3 * 4 - 12]      # no clamping: below the maximal box
    assert res["bb_max"] == [10 * 4 - 7 + 12, 8 * 4 + 3 + 12, 7 * 4 + 12]
    assert res["bb_dims"] == [45, 41, 41]
    empty = ar.auto_bounding_box(views, [ident], 5.0, 9, 4, fused=np.zeros_like(fused))
    assert not empty["found"] and empty["bounds_min"] == [14, 12, 10] and empty["bounds_max"] == [0, 0, 0]


@pytest.fixture(scope="module")
def scene_result():
    views, models, params, truth = ar.scene()
    return views, models, params, truth, ar.auto_bounding_box(views, models, **params)


def test_scene_premise(scene_result):
    """What makes the end-to-end GPU test robust: no voxel of the filtered image lies within
    1 % of the intensity range of the threshold (background <= 1 %, object >= 50 % of the
    range), so a last-bit difference of the fusion cannot move the box."""
    views, models, params, truth, res = scene_result
    assert all(v.shape == (36, 48, 40) for v in views) and len(views) == 3
    assert res["eff_radius"] >= 2 and res["found"]
    rng = float(res["max"]) - float(res["min"])
    assert rng > 0
    fused = res["fused"].astype(np.float64)
    assert (fused[fused < 0.5 * rng + float(res["min"])] <= 0.01 * rng + float(res["min"])).all()
    assert np.abs(res["filtered"].astype(np.float64) - res["threshold"]).min() > 0.01 * rng
    # uncovered voxels exist and are counted: the minimum is their 0
    assert res["min"] == 0 and (res["fused"] == 0).any()


def test_scene_box(scene_result):
    views, models, params, truth, res = scene_result
    for a in range(3):
        assert res["bb_min"][a] <= truth["ellipsoid_min"][a] and truth["ellipsoid_max"][a] <= res["bb_max"][a]
    bead = truth["far_bead"]
    # the bead is in the data that was fused, above the threshold, and outside the box
    ds = params["downsampling"]
    f = [(bead[a] - res["max_min"][a]) // ds for a in range(3)]
    assert res["fused"][f[2], f[1], f[0]] > res["threshold"]
    assert any(not (res["bb_min"][a] <= bead[a] <= res["bb_max"][a]) for a in range(3))
    # without the filter the bead would have been inside
    lo, hi, _ = ar.threshold_bounds(res["fused"], res["threshold"])
    assert all(lo[a] <= f[a] <= hi[a] for a in range(3))
