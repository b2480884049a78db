"""The cases of tests/psf_cases.py have the properties that tests/test_gpu_psf_edges.py
relies on -- proved on the oracle and NumPy alone, no GPU.  A premise that fails means the
case is wrong, not the kernel."""
import numpy as np
import pytest

import psf_cases as pc
from oracle import psf_ref as pr

# share of the normalised PSF's voxels that "always take the fast branch" changes, per
# large-coordinate class, measured on the oracle (70 beads)
MUTANT_SHARE = {"large28": 0.143, "large29": 0.700, "large30": 0.507, "neglarge30": 0.655}


@pytest.mark.parametrize("n", [pc.N_MANY, pc.N_FEW])
@pytest.mark.parametrize("name", sorted(pc.BEAD_CLASSES))
def test_bead_classes_reach_their_branch(name, n):
    """Recomputes the kernel's `q - k == c` and inside tests per (bead, voxel)."""
    img, locs = pc.beads(name, n)
    exact, inside = pc.branch_masks(img.shape, locs, pc.PSF)
    if name == "interior":
        assert exact.all() and inside.all()                       # the fast branch alone
    elif name in ("unit", "below_pow2"):
        assert (~exact).mean() > 0.3                              # the slow branch by the exactness test
    elif name in pc.LARGE_CLASSES:
        assert 0.25 < (~exact).mean() < 0.6 and exact.any()
        assert np.abs(locs).max() + max(pc.PSF) // 2 + 1 < 2 ** 31 - 2
    elif name != "repeat":                                        # exact sums across the border
        assert exact.all() and (~inside).mean() > 0.3
    if name == "last":
        assert all((locs[:, d] == pc.IMG_DIMS[d] - 1).any() for d in range(3))
    if name == "integer":
        assert (locs == np.floor(locs)).all()
    if name == "negfrac":
        assert (locs < 0).all() and (locs != np.floor(locs)).all() and (np.floor(locs) != np.trunc(locs)).all()
    if name == "periods":
        assert (locs < -2 * 12).any() and (locs > 3 * 12).any()
    if name == "repeat":
        assert (locs == locs[0]).all()


@pytest.mark.parametrize("size", [pc.PSF] + pc.SIZES)
def test_mixed_case_has_every_branch(size):
    img, locs = pc.beads("mixed")
    exact, inside = pc.branch_masks(img.shape, locs, size)
    assert (exact & ~inside).any()
    if max(size) > 1:
        assert (~exact).any()
    if min(size) > 1:
        assert (exact & inside).any()


@pytest.mark.parametrize("name", pc.LARGE_CLASSES + ["mixed"])
def test_fast_branch_equals_oracle_where_the_kernel_takes_it(name):
    """The claim of the kernel's comment: where every k + c is exact, the bead's eight
    weights on base floor(c) + k give the bits of nlinear at k + c."""
    img, locs = pc.beads(name)
    exact, _ = pc.branch_masks(img.shape, locs, pc.PSF)
    fast, want = pc.fast_branch_samples(img, locs, pc.PSF), pc.oracle_samples(img, locs, pc.PSF)
    assert exact.any()
    np.testing.assert_array_equal(fast[exact], want[exact])


@pytest.mark.parametrize("name", pc.LARGE_CLASSES)
def test_always_fast_mutant_is_unmistakable(name):
    """The bead's own weights forced on every sample (periodic gather) change the normalised
    PSF in a large share of its voxels, asserted at half the measured share: at these
    coordinates nlinear's weights and base are not the bead's.  This pins nlinear_at, not
    the kernel's branch, which needs the footprint inside the image (see the tie case)."""
    img, locs = pc.beads(name)
    exact, _ = pc.branch_masks(img.shape, locs, pc.PSF)
    fast, want = pc.fast_branch_samples(img, locs, pc.PSF), pc.oracle_samples(img, locs, pc.PSF)
    differ = (fast != want)[~exact].mean()
    share = (pc.psf_of_samples(fast) != pc.psf_of_samples(want)).mean()
    print(f"{name}: inexact {(~exact).mean():.3f}, of which differing {differ:.3f}, PSF voxels changed {share:.3f}")
    assert differ > 0.2
    assert share >= MUTANT_SHARE[name] / 2
    # and with 7 beads (k_psf_extract)
    img, locs = pc.beads(name, pc.N_FEW)
    assert (pc.fast_branch_samples(img, locs, pc.PSF) != pc.oracle_samples(img, locs, pc.PSF)).mean() > 0.05


TIE_SHARE = 0.079   # measured share of the normalised PSF's voxels that the mutant changes


def test_tie_case_sees_the_exactness_test_inside_the_image():
    """The kernel takes the fast branch only with the footprint inside the image, where no
    coordinate is large: the large-coordinate classes above run nlinear_at alone, and a
    kernel without the exactness test passes them.  The tie case has inexact sums inside
    the image whose float32 samples differ."""
    img, locs = pc.tie_case()
    exact, inside = pc.branch_masks(img.shape, locs, pc.PSF)
    assert inside.all() and 0 < (~exact).sum() and exact[np.arange(len(locs)) != len(locs) // 2].all()
    want, mut = pc.oracle_samples(img, locs, pc.PSF), pc.mutant_samples(img, locs, pc.PSF)
    np.testing.assert_array_equal(mut[exact], want[exact])
    share = (pc.psf_of_samples(mut) != pc.psf_of_samples(want)).mean()
    print(f"tie case: inexact samples {(~exact).sum()}, differing {(mut != want).sum()}, PSF voxels changed {share:.3f}")
    assert share >= TIE_SHARE / 2 and share > 0.02
    for name in pc.LARGE_CLASSES:                                  # blind, as said above
        img, locs = pc.beads(name)
        np.testing.assert_array_equal(pc.mutant_samples(img, locs, pc.PSF), pc.oracle_samples(img, locs, pc.PSF))


def test_generic_beads_cannot_see_the_branch():
    """Why the large coordinates are needed: on beads uniform in an ordinary view the forced
    fast branch gives the oracle's float32 bits on every sample."""
    img = pc.image(pc.BIG_DIMS, 2)
    locs = np.random.default_rng(300).uniform([0, 0, 0], pc.BIG_DIMS, size=(300, 3))
    np.testing.assert_array_equal(pc.fast_branch_samples(img, locs, pc.PSF), pc.oracle_samples(img, locs, pc.PSF))


def test_batched_oracle_equals_the_loop():
    img, locs = pc.beads("mixed")
    np.testing.assert_array_equal(pr.extract_psf_local_batched(img, locs, pc.PSF, chunk=16),
                                  pr.extract_psf_local(img, locs, pc.PSF))


def test_c2_tiling_equals_the_plain_oracle():
    img, locs = pc.c2_case()
    exact, _ = pc.branch_masks(img.shape, locs, (21, 21, 23))
    assert exact.all()                                            # dyadic: 100 % exact
    assert len(locs) == pc.C2_BEADS > 2 ** 26 // int(np.prod(pc.C2_SIZE)) == 63
    want = pc.expected_psf(img, locs, (21, 21, 23))
    np.testing.assert_array_equal(pc.c2_expected((21, 21, 23)), want)
    assert np.isfinite(want).all() and len(np.unique(want)) > 30


@pytest.mark.parametrize("case", range(len(pc.EXTREMES)))
def test_extremes_sit_where_stated(case):
    size, imin, imax = pc.EXTREMES[case]
    img, locs = pc.extremes_case(size, imin, imax)
    raw = pr.extract_psf_local(img, locs, size).reshape(-1)
    n = raw.size
    assert int(np.argmin(raw)) == imin % n and int(np.argmax(raw)) == imax % n
    assert (raw == raw.min()).sum() == 1 and (raw == raw.max()).sum() == 1
    exact, inside = pc.branch_masks(img.shape, locs, size)
    assert exact.all() and inside.all()


@pytest.mark.parametrize("kind", pc.SPECIALS)
def test_special_images_give_what_java_gives(kind):
    """oracle.normalize against ExtractPSF.normalize (:277-295) written as its loop."""
    img, locs = pc.special_image(kind), pc.beads("mixed")[1]
    raw = pr.extract_psf_local_batched(img, locs, pc.PSF)
    mn, mx = np.finfo(np.float64).max, -np.finfo(np.float64).max
    for v in raw.reshape(-1).astype(np.float64):
        if v < mn:
            mn = v
        if v > mx:
            mx = v
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        want = ((raw.astype(np.float64) - mn) / (mx - mn)).astype(np.float32)
    got = pr.normalize(raw)
    np.testing.assert_array_equal(got, want)
    if kind == "nan":
        assert 0 < np.isnan(got).sum() < got.size and np.nanmax(got) == 1.0 and np.nanmin(got) == 0.0
    elif kind == "constant":
        assert np.isnan(got).all()
    else:
        assert np.isnan(got).any() and not np.isfinite(raw).all()


def test_normalize_extremes_of_one_value():
    for v in (np.inf, -np.inf, 2.5):
        assert np.isnan(pr.normalize(np.full((1, 1, 1), v, np.float32))).all()


# ------------------------------------------------------------------ E. analytic references vs the oracle
def _psf(shape, seed=61):
    return np.random.default_rng(seed).random(shape).astype(np.float32)


@pytest.mark.parametrize("perm,signs", pc.PERMUTATIONS)
def test_permutation_reference_agrees_with_oracle(perm, signs):
    p = _psf((11, 7, 5))
    for t in [(0, 0, 0), (5, -3, 40)]:
        np.testing.assert_array_equal(pr.transform_psf(p, pc.signed_permutation(perm, signs, t)),
                                      pc.permuted(p, perm, signs))
    assert any(np.linalg.det(pc.signed_permutation(q, s)[:, :3]) < 0 for q, s in pc.PERMUTATIONS)


@pytest.mark.parametrize("axis,shape", pc.SCALE2_CASES)
def test_scale2_reference_agrees_with_oracle(axis, shape):
    p = _psf(shape)
    np.testing.assert_array_equal(pr.transform_psf(p, pc.scale2_model(axis)), pc.scale2_expected(p, axis))


@pytest.mark.parametrize("size", [(9, 9, 11), (8, 10, 12)])
def test_delta_reference_agrees_with_oracle(size):
    for m in pc.delta_models():
        out = pr.transform_psf(pc.delta(size), m)
        c = tuple(n // 2 for n in out.shape)
        assert np.unravel_index(np.argmax(out), out.shape) == c
        assert out[c] >= np.nextafter(np.float32(1), np.float32(0)) and (out == out[c]).sum() == 1
    dets = [np.linalg.det(m[:, :3]) for m in pc.delta_models()]
    assert min(dets) < 0 < max(dets) and any((m[:, 3] != np.floor(m[:, 3])).all() for m in pc.delta_models())


def test_size_rule_reference_agrees_with_oracle():
    for scales, want in pc.SIZE_RULE:
        m = np.hstack([np.diag(scales), np.array([[3.0], [-2.5], [0.0]])])
        new, off = pr.transformed_size((11, 11, 11), m)
        assert tuple(new) == want
        assert off == [s * 5 + t - n // 2 for s, t, n in zip(scales, (3.0, -2.5, 0.0), want)]


def test_even_sizes_under_identity():
    """transformPSF (:326-343) on 8 x 10 x 12: extents 7, 9, 11 -> 8, 10, 12 -> odd 9, 11, 13;
    centre size / 2 = 4, 5, 6 = newSize / 2, offset 0: the input, zero-padded by one at the
    upper end of every axis."""
    p = _psf((12, 10, 8))
    want = np.zeros((13, 11, 9), np.float32)
    want[:12, :10, :8] = p
    np.testing.assert_array_equal(pr.transform_psf(p, pc.IDENT), want)


# ------------------------------------------------------------------ G
@pytest.mark.parametrize("shape", pc.PROJECTION_SHAPES)
def test_max_projection_oracle_follows_the_java_loop(shape):
    v = pc.projection_volume(shape)
    for d in (-1, 0, 1, 2):
        got, used = pr.max_projection(v, d)
        want, wused = pc.java_max_projection(v, d)
        assert used == wused
        np.testing.assert_array_equal(got, want)
        assert np.isneginf(want).any() and not np.isnan(want).any()
    assert pr.max_projection(np.zeros((5, 5, 5), np.float32))[1] == 0      # ties: the first wins
    assert pr.max_projection(np.zeros((4, 4, 6), np.float32))[1] == 1
