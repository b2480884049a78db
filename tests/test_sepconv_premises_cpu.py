"""The premises of tests/test_gpu_sepconv_edges.py, proved without a GPU: the plain
reference of tests/sepconv_cases.py agrees with the oracle where the oracle is defined,
is anchored to a float64 sum by a derived bound, follows the index rule of
csrc/sepconv.hpp on axes shorter than the reach -- and the cases can tell the mistakes
they are there for (reversed taps, a wrong mode, skipped zero taps, the dispatch route)."""
import numpy as np
import pytest

import sepconv_cases as sc
from conftest import rel_l2
from oracle import dog_ref
from spim_registration_amd import legacy


@pytest.mark.parametrize("K", [7, 63])
@pytest.mark.parametrize("mode", sc.MODES)
def test_ref3d_equals_the_oracle_on_finite_input(K, mode):
    """Written independently, bit for bit the same: random taps, and padded Gaussians
    (whose zero taps the oracle skips and ref_pass adds as +-0)."""
    img = sc.volume((11, 13, 17), 1)
    for ks in (sc.random_taps(K, 2), legacy.get_cuda_kernels([1.0, 0.8, 0.6] if K == 7 else [6.0, 3.0, 9.5])):
        assert len(ks[0]) == K
        got = sc.ref3d(img, ks, mode, sc.OOB_VALUE)
        exp = dog_ref.gauss3d(img, ks, sc.MODE_NAMES[mode], sc.OOB_VALUE)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("K", sc.TAP_COUNTS)
def test_ref_pass_within_the_derived_bound_of_float64(K):
    """|out32 - out64| <= gamma_(K + 1) * sum |v k| (sepconv_cases.pass_bound), every axis
    and mode; and the bound is tight enough to notice one dropped tap."""
    img = sc.volume((9, 10, 140), 3)
    ks = sc.random_taps(K, 4)
    for axis in range(3):
        for mode in sc.MODES:
            out = sc.ref_pass(img, ks[axis], axis, mode, sc.OOB_VALUE)
            o64, mag = sc.ref_pass64(img, ks[axis], axis, mode, sc.OOB_VALUE)
            assert o64.dtype == np.float64
            assert np.all(np.abs(out.astype(np.float64) - o64) <= sc.pass_bound(K, mag))
    o64, mag = sc.ref_pass64(img, ks[0], 0, sc.MIRROR)
    dropped = ks[0].copy()
    dropped[K // 2 + 1] = 0
    bad = sc.ref_pass(img, dropped, 0, sc.MIRROR)
    assert np.mean(np.abs(bad.astype(np.float64) - o64) > sc.pass_bound(K, mag)) > 0.9


def _extended_line(line, reach, mode, value):
    """``line`` with ``reach`` samples added at each end, built sample by sample by
    walking outwards (mirror: bouncing between the ends without repeating them)."""
    n = len(line)
    left, right = [], []
    if mode in (sc.ZERO, sc.VALUE):
        fill = np.float32(value if mode == sc.VALUE else 0.0)
        left = right = [fill] * reach
    elif mode == sc.BORDER:
        left, right = [line[0]] * reach, [line[-1]] * reach
    else:
        for start, step, dst in ((0, -1, left), (n - 1, 1, right)):
            pos, dirn = start, step
            for _ in range(reach):
                if n > 1:
                    if not 0 <= pos + dirn < n:
                        dirn = -dirn
                    pos += dirn
                dst.append(line[pos])
        left = left[::-1]
    return np.array(list(left) + list(line) + list(right), np.float32)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("mode", sc.MODES)
def test_index_rule_on_axes_shorter_than_the_reach(n, mode):
    """Reach 63 (127 taps) over 1, 2 or 3 samples: mirror folds up to 63 times."""
    K, r = 127, 63
    line = np.float32([3.0, 5.0, 11.0][:n])
    ext = _extended_line(line, r, mode, sc.OOB_VALUE)
    assert len(ext) == n + 2 * r
    src, outside = sc.source_index(np.arange(-r, n + r), n, mode)
    got = np.where(outside, np.float32(sc.OOB_VALUE if mode == sc.VALUE else 0.0), line[src])
    np.testing.assert_array_equal(got, ext)
    if mode == sc.MIRROR and n == 3:
        np.testing.assert_array_equal(ext[r - 5:r], np.float32([5, 3, 5, 11, 5]))   # ... 1 0 1 2 1 | 0 1 2
    taps = sc.random_taps(K, 5)[0]
    for axis in range(3):
        shape = [1, 1, 1]
        shape[2 - axis] = n
        out = sc.ref_pass(line.reshape(shape), taps, axis, mode, sc.OOB_VALUE).reshape(-1)
        for i in range(n):
            acc = np.float32(0)
            for j in range(K):
                acc = np.float32(acc + np.float32(ext[i + j] * taps[j]))
            assert out[i] == acc


@pytest.mark.parametrize("K", sc.TAP_COUNTS)
def test_reversed_taps_are_visible(K):
    """At every tap count the reference under reversed taps is far from the reference:
    a kernel that runs the taps backwards cannot pass the bit-exact comparison."""
    shape, seed = sc.ALL_TAPS_SHAPE, sc.ALL_TAPS_SEED
    ks = sc.random_taps(K, sc.all_taps_seed(K))
    for a in range(3):
        assert np.abs(ks[a] - ks[a][::-1]).max() > 0.1
        assert np.abs(ks[a] - ks[(a + 1) % 3]).max() > 0.1      # (and swapped axes)
    for mode in (sc.ZERO, sc.MIRROR):
        exp = sc.expected(shape, seed, K, sc.all_taps_seed(K), mode)
        rev = sc.ref3d(sc.volume(shape, seed), [k[::-1] for k in ks], mode, sc.OOB_VALUE)
        assert rel_l2(rev, exp) > 1e-2
    for axis in range(3):      # a single reversed pass too (the window form is per axis)
        img = sc.volume((20, 21, 22), 6)
        one = sc.ref_pass(img, ks[axis], axis, sc.BORDER)
        assert rel_l2(sc.ref_pass(img, ks[axis][::-1], axis, sc.BORDER), one) > 1e-2


@pytest.mark.parametrize("shape", sc.SEAM_SHAPES + [sc.ALL_TAPS_SHAPE])
def test_modes_differ_at_each_seam_shape(shape):
    """The four modes give four different results at every seam shape, each pair apart
    in at least every hundredth voxel, so a kernel that confuses two modes cannot pass."""
    K = 15
    ks = sc.random_taps(K, 7)
    img = sc.volume(shape, sc.SEAM_SEED)
    outs = [sc.ref3d(img, ks, m, sc.OOB_VALUE) for m in sc.MODES]
    for a in range(4):
        for b in range(a + 1, 4):
            assert np.mean(outs[a] != outs[b]) > 0.01, (a, b)


def test_single_pass_modes_differ_on_the_fallback_shapes():
    """Per pass of the fallback cases: BORDER and MIRROR differ along every axis of more
    than one sample (on a single sample they coincide, as they must), VALUE from both."""
    for w, h, d in sc.FALLBACK_WHD:
        img = sc.volume((d, h, w), sc.FALLBACK_SEED)
        for axis, n in enumerate((w, h, d)):
            k = sc.random_taps(15, 8)[axis]
            b, m, v = (sc.ref_pass(img, k, axis, mode, sc.OOB_VALUE) for mode in (sc.BORDER, sc.MIRROR, sc.VALUE))
            assert np.array_equal(b, m) == (n == 1)
            assert not np.array_equal(b, v) and not np.array_equal(m, v)
    # the routes the cases are there for (csrc/sepconv.hip's dispatch condition)
    assert [sc.tiled((2, 1, 65536), a) for a in range(3)] == [False, False, True]
    assert [sc.tiled((1, 65536, 2), a) for a in range(3)] == [False, True, False]
    assert all(sc.tiled(s[::-1], a) for s in sc.SEAM_SHAPES + [sc.ALL_TAPS_SHAPE] for a in range(3))


def test_nan_footprint_of_all_taps_differs_from_the_zero_skipping_oracle():
    """A padded 15-tap Gaussian has genuine zero taps; 0 * NaN and 0 * inf are NaN, so
    visiting every tap spreads a non-finite value over the whole padded footprint,
    which the oracle's skip of zero taps does not."""
    ks = legacy.get_cuda_kernels(sc.NONFINITE_SIGMAS)
    assert all(len(k) == 15 and (k == 0).sum() >= 4 for k in ks)
    img = sc.nonfinite_volume()
    assert np.isnan(img).sum() == 1 and np.isinf(img).sum() == 1
    allt = sc.ref3d(img, ks, sc.MIRROR)
    with np.errstate(invalid="ignore"):
        skip = dog_ref.gauss3d(img, ks, "mirror")
    assert np.isnan(allt).sum() > np.isnan(skip).sum() > 0
    assert np.all(np.isnan(allt) | ~np.isnan(skip))            # the skipping footprint lies inside
    finite = ~np.isnan(allt)
    np.testing.assert_array_equal(allt[finite], skip[finite])  # and away from it nothing changes


def test_dog_cases_take_the_routes_they_name():
    """The tap classes of the DoG cases, and the shapes that leave the fused route."""
    assert [sc.dog_taps(s) for s, _ in sc.DOG_TALL_SIGMAS] == [k for _, k in sc.DOG_TALL_SIGMAS]
    assert sc.dog_taps(sc.DOG_127_SIGMA) == 127
    assert sc.dog_taps(17.0) == 127 and sc.dog_taps(sc.DOG_REFUSED_SIGMA) is None
    assert sc.DOG_TALL_SHAPE[0] > sc.GRID_LIMIT and sc.DOG_LONG_SHAPE[1] > sc.GRID_LIMIT * 32
    # the tall volume: x and y passes fall back, z is tiled; the long one: y tiled only
    assert [sc.tiled(sc.DOG_TALL_SHAPE[::-1], a) for a in range(3)] == [False, False, True]
    assert [sc.tiled(sc.DOG_LONG_SHAPE[::-1], a) for a in range(3)] == [False, True, False]
