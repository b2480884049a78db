"""The content-based weight passes of csrc/content_weights.hip at their edges: the seams
of the 128-output tiles along every axis, the tap chunking on both sides of every multiple
of 16 up to the 463-tap limit, the grid stride and the tail of the min / max reduction, and
non-finite input -- bit for bit against the operation-order restatement of
tests/content_cases.py (its premises: tests/test_content_premises_cpu.py).

Where each branch of the kernels runs (shapes (nz, ny, nx)):
  k_gauss_pass<true>, nat > 1, p0 > 0      test_seams nx 129, 257; test_all_axes_over_a_seam;
                                           test_tap_counts, test_longest_kernel (nx 140)
  k_gauss_pass<false>, nat > 1, p0 > 0     test_seams ny / nz 129, 257 (the strided store
                                           out[col + (p0 + q0 + j) * pstride]); test_all_axes_over_a_seam
  a short last tile (q0 >= tile)           lengths 1, 2, 127 (one tile), 129, 257 (one output in the last)
  a last line block of one line            every seam case: 65 rows, or nx = 65
  the tail step alone (kpad 16)            test_tap_counts 3, 5, 15; the reduction and non-finite cases
  whole loop turns alone (kpad 32, 64)     17, 31, 49; sigma 3 (19 taps)
  loop turns and the tail (kpad 48, 464)   33, 47; sigma 6 (37 taps); 463 (14 turns and the tail)
  the largest LDS request, 64 x 593        test_longest_kernel
  check_content_sigmas at the limit        test_tap_limit
  k_minmax_partial: one partial block      test_fewer_voxels_than_one_block
    second round, ragged last block        test_maximum_in_the_last_partial_block, test_minimum_in_the_second_round
  k_normalise skipped                      1 voxel; test_non_finite_input
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import content_cases as cc
from spim_registration_amd import _lib
from spim_registration_amd.input_prep import content_based_weights, content_tile_sizes, fuse_weighted_average

pytestmark = pytest.mark.gpu

ERR_ARG = -1   # SPIMDECON_ERR_ARG, include/spimdecon.h


def run(name, img=None):
    c = cc.CASES[name]
    got = content_based_weights(cc.image(name) if img is None else img, c.s1, c.s2)
    assert got.dtype == np.float32 and got.shape == c.shape
    return got


def check(name):
    want = cc.weights(name)
    np.testing.assert_array_equal(run(name), want)
    return want


def test_tile_sizes_are_the_ones_the_cases_straddle(gpu):
    """The constants the cases of tests/content_cases.py are built around, as the library
    reports them (csrc/content_weights.hip, the constexpr block at the head of the file:
    kCwTile = kCwOut * (kCwBlock / 64) = 128 outputs per line and block, kCwLines = 64 lines
    per block, kCwChunk = 16 taps per window step, kCwMaxTaps = 463, kRedBlock = 256 and
    kRedGrid = 1024).  Whoever changes the tiling moves the seams: revisit SEAM_LENGTHS,
    TAP_COUNTS and the reduction shapes."""
    assert content_tile_sizes() == (cc.TILE, cc.LINES, cc.CHUNK, cc.MAX_TAPS, cc.RED_BLOCK,
                                    cc.RED_ROUND // cc.RED_BLOCK)
    assert (cc.TILE, cc.LINES, cc.CHUNK, cc.MAX_TAPS, cc.RED_ROUND) == (128, 64, 16, 463, 262144)


# ------------------------------------------------------------------ a. seams
@pytest.mark.parametrize("n", cc.SEAM_LENGTHS)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_seams(gpu, axis, n):
    """1, 2, 127, 128, 129 and 257 samples along one axis, sigma 3 and 6 (19 and 37 taps);
    the x pass over 65 rows, the y and z passes over 65 columns and 3 along the third axis."""
    check(cc.seam_name(axis, n))


def test_all_axes_over_a_seam(gpu):
    """(130, 131, 129): every pass has two tiles along its axis and ragged line blocks."""
    check("seam_all")


def test_seam_volume_inside_fusion(gpu):
    """The same volume as the one view of a weighted-average fusion with the identity model:
    (v * w) / w in double is v where w > 0 and the output is 0 where w == 0
    (test_gpu_content.test_weights_inside_fusion_are_the_stand_alone_weights), so the fusion
    call ran the passes at p0 > 0 along x, y and z and normalised with the same pair."""
    name = "seam_all"
    img, c, w = cc.image(name), cc.CASES[name], cc.weights(name)
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    dims = (img.shape[2], img.shape[1], img.shape[0])
    got = fuse_weighted_average([img], [ident], (0, 0, 0), dims, use_blending=False, use_content_based=True,
                                content_sigma1=c.s1, content_sigma2=c.s2)
    assert (w == 0).sum() == 1
    np.testing.assert_array_equal(got, np.where(w > 0, img, np.float32(0)))


# ------------------------------------------------------------------ b. tap counts
@pytest.mark.parametrize("r", range(len(cc.TAP_COUNTS)))
def test_tap_counts(gpu, r):
    """3, 5, 15, 17, 31, 33, 47 and 49 taps: rotation r gives the six slots (sigma1 x, y, z,
    sigma2 x, y, z) six different counts, so a swapped axis or sigma set changes the result
    (premises: test_mutant_swapped_sigmas); every count meets every slot over the eight."""
    name = f"taps_r{r}"
    c = cc.CASES[name]
    assert [len(cc.taps(s)) for s in c.s1 + c.s2] == cc.rotation_taps(r)
    check(name)


@pytest.mark.parametrize("name", ["taps_max_s2", "taps_max_s1"])
def test_longest_kernel(gpu, name):
    """463 taps on all three axes of one blur over (6, 7, 140): reach 231 over 6 and 7
    samples (the mirror folds some 40 times), 29 chunks, the largest LDS request."""
    c = cc.CASES[name]
    assert sorted(len(cc.taps(s)) for s in c.s1 + c.s2) == [3, 3, 3] + [cc.MAX_TAPS] * 3
    check(name)


def _sigmas(slot, value):
    s = [2.0] * 6
    s[slot] = value
    return (C.c_double * 3)(*s[:3]), (C.c_double * 3)(*s[3:])


@pytest.mark.parametrize("slot", range(6))
def test_tap_limit(gpu, lib, slot):
    """463 taps are served and 465 refused with ERR_ARG and a message naming the limit, in
    each of the six sigma slots."""
    img = cc.volume((4, 5, 6), 5000 + slot)
    out = np.full_like(img, -7)
    dims = (C.c_int64 * 3)(6, 5, 4)
    s1, s2 = _sigmas(slot, cc.sigma_for_taps(cc.MAX_TAPS))
    assert lib.spim_content_based_weights(img.ctypes.data, dims, s1, s2, out.ctypes.data, 0) == 0, _lib.last_error()
    np.testing.assert_array_equal(out, cc.ref_weights(img, tuple(s1), tuple(s2)))
    s1, s2 = _sigmas(slot, cc.sigma_for_taps(cc.MAX_TAPS + 2))
    before = out.copy()
    assert lib.spim_content_based_weights(img.ctypes.data, dims, s1, s2, out.ctypes.data, 0) == ERR_ARG
    assert str(cc.MAX_TAPS) in _lib.last_error() and "taps" in _lib.last_error()
    np.testing.assert_array_equal(out, before)


def test_tap_limit_in_the_fusion_call(gpu, lib):
    img = cc.volume((4, 5, 6), 5010)
    out = np.empty_like(img)
    view = (_lib.ViewSource * 1)()
    view[0].img = _lib.fptr(img)
    view[0].dims[:] = [6, 5, 4]
    view[0].model[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    p = _lib.FusionParams()
    lib.spim_fusion_params_default(C.byref(p))
    p.bb_dims[:] = [6, 5, 4]
    p.use_blending = 0
    fuse = lib.spim_fuse_weighted_average_content
    s1, s2 = _sigmas(4, cc.sigma_for_taps(cc.MAX_TAPS))
    assert fuse(1, view, C.byref(p), None, None, s1, s2, _lib.fptr(out)) == 0, _lib.last_error()
    w = cc.ref_weights(img, tuple(s1), tuple(s2))
    np.testing.assert_array_equal(out, np.where(w > 0, img, np.float32(0)))
    s1, s2 = _sigmas(4, cc.sigma_for_taps(cc.MAX_TAPS + 2))
    assert fuse(1, view, C.byref(p), None, None, s1, s2, _lib.fptr(out)) == ERR_ARG
    assert str(cc.MAX_TAPS) in _lib.last_error()


# ------------------------------------------------------------------ c. the reduction
@pytest.mark.parametrize("name", ["red_1", "red_2", "red_30"])
def test_fewer_voxels_than_one_block(gpu, name):
    """1, 2 and 30 voxels: one partial block, most of its threads without a voxel.  One
    voxel: the range is 0, the normalisation is skipped and the blurred square comes back."""
    want = check(name)
    if name == "red_1":
        assert want is cc.raw(name)
    else:
        assert want.min() == 0.0 and want.max() == 1.0


def test_maximum_in_the_last_partial_block(gpu):
    """266,175 voxels, the unique maximum at the far corner, among the 191 voxels after the
    last whole block of 256 and in the second round of the grid stride (premises:
    test_reduction_cases_place_the_extrema_where_they_can_be_missed)."""
    want = check("red_tail")
    assert want.reshape(-1)[-1] == 1.0


def test_minimum_in_the_second_round(gpu):
    """528,320 voxels, the unique minimum past the first 262,144."""
    want = check("red_second_round")
    assert int(want.argmin()) >= cc.RED_ROUND and want.min() == 0.0


# ------------------------------------------------------------------ d. non-finite input
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_input(gpu, value):
    """One NaN or +inf at the centre of 70^3 under 3-tap kernels.  The range is NaN, so the
    output is not normalised.  The Gaussians reach R1 + R2 = 2 voxels: that box is non-finite.
    The kernels also multiply the zero taps that pad each kernel to 16 (0 * NaN = 0 * inf =
    NaN), over as many further positions as the voxel's place in its 128-output tile lets
    them see: at most 15 per pass, so outside the box of half-width 2 + 2 * 15 the output is
    the clean image's blurred square bit for bit.  The shell between the boxes is
    unspecified (content-based weights)."""
    got = run("nonfinite", cc.nonfinite_volume(value))
    clean = cc.raw("nonfinite")
    shape = clean.shape
    inner, outer = cc.box(shape, cc.NONFINITE_AT, cc.NONFINITE_INNER), cc.box(shape, cc.NONFINITE_AT, cc.NONFINITE_OUTER)
    assert not np.isfinite(got[inner]).any()
    np.testing.assert_array_equal(got[~outer], clean[~outer])
    assert not np.array_equal(cc.weights("nonfinite")[~outer], clean[~outer])     # (so: not normalised)
