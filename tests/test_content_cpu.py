"""CPU: the content-based-weights restatement (tests/content_ref.py) against an
independently computed fixture, the sigma rule of ProcessFusion.getContentBased,
and the C-ABI of the mode (header, exports, binding)."""
import ctypes as C
import os

import numpy as np
import pytest

import content_ref as cr
from oracle import fusion_ref as fr
from spim_registration_amd import _lib
from spim_registration_amd.input_prep import content_based_sigmas

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "content_based.npz"))

# The fixture is a direct float64 sum, the restatement a float64 FFT; both round c to
# float32 after each blur.  Where the two float64 values straddle a rounding boundary c
# (<= 64) moves by one ulp, 3.8e-6; d = c - I (|d| <~ 5) then moves d^2 by 2 * 5 * 3.8e-6
# = 3.8e-5 against a maximum of ~25 that the normalisation maps to 1: 1.5e-6 on the
# weight, plus 6e-8 per float32 rounding after it.
GOLDEN_ATOL = 5e-6


def test_restatement_matches_direct_sum_fixture():
    w = cr.content_weights(GOLD["img"], GOLD["sigma1"], GOLD["sigma2"], "f64")
    want = GOLD["weights"]
    assert w.dtype == np.float32 and w.shape == want.shape
    assert want.min() == 0.0 and want.max() == 1.0 and w.min() == 0.0 and w.max() == 1.0
    assert 0.05 < want.std()                       # a structured weight image, not a constant
    np.testing.assert_allclose(w, want, rtol=0, atol=GOLDEN_ATOL)


def test_restatement_f32_stand_in_is_close():
    w64 = cr.content_weights(GOLD["img"], GOLD["sigma1"], GOLD["sigma2"], "f64")
    w32 = cr.content_weights(GOLD["img"], GOLD["sigma1"], GOLD["sigma2"], "f32")
    d32 = float(np.abs(w32.astype(np.float64) - w64).max())
    assert 0 < d32 < 1e-5


def test_constant_image_is_not_normalised():
    """normalizeImage returns without touching the image when max - min is 0."""
    w = cr.content_weights(GOLD["flat"], GOLD["sigma1"], GOLD["sigma2"], "f64")
    np.testing.assert_array_equal(w, GOLD["flat_weights"])
    assert w.min() == w.max()
    flat = np.full((2, 3, 4), 3.0, np.float32)
    assert cr.normalize_image(flat) is not None and (cr.normalize_image(flat) == 3.0).all()
    nan = flat.copy()
    nan[0, 0, 0] = np.nan
    np.testing.assert_array_equal(cr.normalize_image(nan), nan)
    inf = flat.copy()
    inf[1, 2, 3] = np.inf
    np.testing.assert_array_equal(cr.normalize_image(inf), inf)


def test_kernel_is_the_float_of_the_double_product():
    k = cr.gaussian_kernel_3d((1.2, 1.0, 0.8))
    assert k.shape == (5, 7, 9) and k.dtype == np.float32       # [z, y, x] sizes for sigma (x, y, z)
    assert abs(float(k.astype(np.float64).sum()) - 1.0) < 1e-6
    assert cr.gaussian_kernel_3d((20, 20, 20)).shape == (121, 121, 121)
    assert cr.gaussian_kernel_3d((40, 40, 2)).shape == (13, 241, 241)


@pytest.mark.parametrize("voxel,s1,s2", [
    # (1, 1, 3): min 1, axes 0 and 1 divided by 1 -> unchanged; z is never adjusted
    ((1, 1, 3), [20.0, 20.0, 20.0], [40.0, 40.0, 40.0]),
    # (2, 1, 1): min 1, axis 0 divided by 2 / 1
    ((2, 1, 1), [10.0, 20.0, 20.0], [20.0, 40.0, 40.0]),
    # (1, 2, 0.5): min 0.5, axis 0 divided by 2, axis 1 by 4, axis 2 (the finest) untouched
    ((1, 2, 0.5), [10.0, 5.0, 20.0], [20.0, 10.0, 40.0]),
])
def test_content_based_sigmas(voxel, s1, s2):
    for fn in (content_based_sigmas, cr.content_based_sigmas):
        g1, g2 = fn(voxel)
        assert list(g1) == s1 and list(g2) == s2
        g1, g2 = fn(voxel, adjust=False)
        assert list(g1) == [20.0] * 3 and list(g2) == [40.0] * 3
    g1, g2 = content_based_sigmas((2, 1, 1), (6, 6, 6), (9, 12, 15))
    assert g1 == [3.0, 6.0, 6.0] and g2 == [4.5, 12.0, 15.0]


def test_fuse_with_unit_content_weights_is_the_blended_fusion():
    """A content weight of 1 everywhere leaves the blended fusion unchanged: with border 0
    the blending weight is already 0 where the zero-extended sampling falls below 1
    (t beyond the last voxel centre)."""
    rng = np.random.default_rng(3)
    srcs = [(rng.random((6, 8, 10)) * 50 + 1).astype(np.float32) for _ in range(2)]
    models = [np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([np.eye(3), [[2.5], [1.25], [-1.5]]])]
    bb_min, bb_dims = (-2, -2, -2), (15, 12, 9)
    borders, ranges = [(0, 0, 0)] * 2, [(3, 3, 2)] * 2
    ones = [np.ones_like(s) for s in srcs]
    got = cr.fuse(srcs, models, ones, bb_min, bb_dims, 1.0, 1, True, borders, ranges)
    want = fr.fuse_weighted_average(srcs, models, bb_min, bb_dims, 1.0, 1, True, borders, ranges)
    np.testing.assert_array_equal(got, want)
    # content weights alone: a view with weight 0 everywhere drops out
    zero = [np.ones_like(srcs[0]), np.zeros_like(srcs[1])]
    alone = cr.fuse(srcs, models, zero, bb_min, bb_dims)
    one_view = cr.fuse(srcs[:1], models[:1], ones[:1], bb_min, bb_dims)
    np.testing.assert_array_equal(alone, one_view)
    assert (alone > 0).any() and (alone == 0).any()


def test_content_symbols_declared_exported_and_bound(lib):
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "spimdecon.h")).read()
    for name in ("spim_content_based_weights", "spim_fuse_weighted_average_content"):
        assert name + "(" in hdr, f"{name} not declared in spimdecon.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    assert "content-based not supported" not in hdr
    assert C.sizeof(_lib.FusionParams) == 2 * 24 + 4 * 6 + 4 * 8      # the struct keeps its size
