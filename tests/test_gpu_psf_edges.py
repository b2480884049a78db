"""csrc/psf.hip at its edges, bit for bit against oracle/psf_ref.py and against references
that do not come from the oracle.  The cases live in tests/psf_cases.py;
tests/test_psf_premises_cpu.py proves what each of them relies on.

Every operation of extraction, normalisation and transformation is an IEEE double or
float add, multiply, divide, floor or conversion in the reference's order on both sides
(the library is built with -ffp-contract=off), so every comparison is assert_array_equal,
NaN positions included."""
import ctypes as C

import numpy as np
import pytest
import torch   # before libspimdecon loads: one HIP runtime in the process (torch's), as in bench.py

import psf_cases as pc
from oracle import psf_ref as pr
from spim_registration_amd import _lib, psf

pytestmark = pytest.mark.gpu

ERR_ARG = -1


def eq(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(got, want)


def check_extract(img, locs, size, model=pc.ROT):
    orig, trans = psf.extract_psf(img, locs, size, model)
    eo, et = pc.expected(img, locs, size, model)
    eq(orig, eo)
    eq(trans, et)
    return orig


# ------------------------------------------------------------------ B. branches of k_psf_samples / nlinear_at
@pytest.mark.parametrize("n", [pc.N_MANY, pc.N_FEW])
@pytest.mark.parametrize("name", sorted(pc.BEAD_CLASSES) + ["mixed"])
def test_bead_classes(gpu, name, n):
    img, locs = pc.beads(name, n)
    orig = check_extract(img, locs, pc.PSF)
    assert np.isfinite(orig).all() and orig.max() == 1.0 and orig.min() == 0.0


def test_exactness_test_inside_the_image(gpu):
    """Inexact k + c with the footprint inside the image and float32 samples that differ
    between nlinear's weights and the bead's (70 of the 891 voxels): the one case that a
    k_psf_samples without `q - k == c` fails.  The large-coordinate classes above never
    reach the fast branch (their footprints are outside) and run nlinear_at alone."""
    img, locs = pc.tie_case()
    check_extract(img, locs, pc.PSF)
    check_extract(img, locs[pc.N_MANY // 2 - 3:pc.N_MANY // 2 + 4], pc.PSF)


@pytest.mark.parametrize("n", [pc.N_MANY, pc.N_FEW])
@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: "x".join(map(str, s)))
def test_psf_sizes_around_the_blocks(gpu, size, n):
    img, locs = pc.beads("mixed", n)
    orig = check_extract(img, locs, size, pc.IDENT)
    assert np.isnan(orig).all() == (size == (1, 1, 1))            # max == min: 0 / 0


# ------------------------------------------------------------------ C. chunk loop, accumulate unroll
@pytest.mark.parametrize("n", pc.C1_COUNTS)
def test_two_bead_chunks(gpu, n):
    """65535 beads (grid.y) and a second chunk of 1 or of 32: the locations offset, acc
    carried from chunk to chunk, remainders 31 and 1 / 31 and 0 of the 32-wide unroll."""
    img, locs = pc.uniform_beads(n)
    check_extract(img, locs, pc.C1_SIZE, pc.IDENT)


@pytest.mark.parametrize("n", pc.SMALL_COUNTS)
def test_unroll_remainders(gpu, n):
    img, locs = pc.uniform_beads(n)
    check_extract(img, locs, pc.PSF)


def test_sample_budget_chunks(gpu):
    """101 x 101 x 103: 2^26 / 1050703 = 63 beads per chunk, 63 + 2.  The expectation is the
    oracle's PSF of one period tiled (test_psf_premises_cpu.py proves the tiling)."""
    img, locs = pc.c2_case()
    try:
        orig, trans = psf.extract_psf(img, locs, pc.C2_SIZE)
        assert trans is None
        eq(orig, pc.c2_expected(pc.C2_SIZE))
    finally:
        psf.release_workspace()                                   # the 265 MB sample buffer


# ------------------------------------------------------------------ D. min / max / normalise
@pytest.mark.parametrize("case", range(len(pc.EXTREMES)))
def test_extremes(gpu, case):
    size, imin, imax = pc.EXTREMES[case]
    img, locs = pc.extremes_case(size, imin, imax)
    orig = check_extract(img, locs, size, pc.IDENT).reshape(-1)
    assert orig[imin] == 0.0 and orig[imax] == 1.0 and (orig == 0).sum() == 1 and (orig == 1).sum() == 1
    many = psf.extract_psf(img, np.tile(locs, (66, 1)), size)[0]  # the two-phase path, same extremes
    eq(many, pc.expected_psf(img, np.tile(locs, (66, 1)), size))
    assert many.reshape(-1)[imin] == 0.0 and many.reshape(-1)[imax] == 1.0


@pytest.mark.parametrize("n", [pc.N_MANY, pc.N_FEW])
@pytest.mark.parametrize("kind", pc.SPECIALS)
def test_nan_inf_and_constant_images(gpu, kind, n):
    img, locs = pc.special_image(kind), pc.beads("mixed", n)[1]
    with np.errstate(invalid="ignore"):
        orig = check_extract(img, locs, pc.PSF)
    if kind == "nan":
        assert 0 < np.isnan(orig).sum() < orig.size and np.nanmax(orig) == 1.0 and np.nanmin(orig) == 0.0
    if kind == "constant":
        assert np.isnan(orig).all()


# ------------------------------------------------------------------ E. the transform
def _psf(shape, seed=61):
    return np.random.default_rng(seed).random(shape).astype(np.float32)


def test_integer_translation_is_the_identity(gpu):
    for shape in [(11, 7, 5), (1, 1, 9), (1, 1, 1)]:
        p = _psf(shape)
        for t in [(0, 0, 0), (5, -3, 40), (-1000, 7, 1)]:
            eq(psf.transform_psf(p, np.hstack([np.eye(3), np.array(t, float)[:, None]])), p)


@pytest.mark.parametrize("perm,signs", pc.PERMUTATIONS)
def test_signed_permutations(gpu, perm, signs):
    p = _psf((11, 7, 5))
    for t in [(0, 0, 0), (5, -3, 40)]:
        eq(psf.transform_psf(p, pc.signed_permutation(perm, signs, t)), pc.permuted(p, perm, signs))


@pytest.mark.parametrize("axis,shape", pc.SCALE2_CASES)
def test_scale_2(gpu, axis, shape):
    p = _psf(shape)
    eq(psf.transform_psf(p, pc.scale2_model(axis)), pc.scale2_expected(p, axis))


@pytest.mark.parametrize("size", [(9, 9, 11), (8, 10, 12)])
def test_delta_stays_at_the_centre(gpu, size):
    for m in pc.delta_models():
        out = psf.transform_psf(pc.delta(size), m)
        c = tuple(n // 2 for n in out.shape)
        assert all(n % 2 == 1 for n in out.shape)
        assert np.unravel_index(np.argmax(out), out.shape) == c and (out == out[c]).sum() == 1
        assert out[c] >= np.nextafter(np.float32(1), np.float32(0))
        eq(out, pr.transform_psf(pc.delta(size), m))


def test_size_rule(gpu):
    """newSize = (int) extent + 1, made odd; offset = model(dim / 2) - newSize / 2."""
    for scales, want in pc.SIZE_RULE:
        tr = (3.0, -2.5, 0.0)
        new, off = psf.transformed_size((11, 11, 11), np.hstack([np.diag(scales), np.array(tr)[:, None]]))
        n = [int(s * 10.0) + 1 for s in scales]
        n = [v + 1 if v % 2 == 0 else v for v in n]
        assert tuple(new) == tuple(n) == want
        assert off == [s * 5.0 + t - v // 2 for s, t, v in zip(scales, tr, n)]


def test_even_sizes_under_identity(gpu):
    """transformPSF on 8 x 10 x 12: odd size 9 x 11 x 13, centre size / 2 kept: the input,
    zero-padded by one at the upper ends."""
    p = _psf((12, 10, 8))
    want = np.zeros((13, 11, 9), np.float32)
    want[:12, :10, :8] = p
    assert psf.transformed_size((8, 10, 12), pc.IDENT) == ([9, 11, 13], [0.0, 0.0, 0.0])
    eq(psf.transform_psf(p, pc.IDENT), want)


@pytest.mark.parametrize("shape", pc.ORACLE_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", sorted(pc.ORACLE_MODELS))
def test_transform_matches_oracle(gpu, name, shape):
    p, m = _psf(shape), pc.ORACLE_MODELS[name]
    size = (shape[2], shape[1], shape[0])
    assert psf.transformed_size(size, m) == tuple(map(list, pr.transformed_size(size, m)))
    eq(psf.transform_psf(p, m), pr.transform_psf(p, m))


def _model12(m):
    return (C.c_double * 12)(*[float(v) for v in np.asarray(m, np.float64).reshape(12)])


@pytest.mark.parametrize("bad", range(1 + len(pc.NONFINITE)))
def test_bad_models_are_errors_and_leave_the_pool_usable(gpu, lib, bad):
    m = ([pc.SINGULAR] + pc.NONFINITE)[bad]
    p = _psf((11, 9, 9))
    size = (C.c_int64 * 3)(9, 9, 11)
    out = np.zeros(64 ** 3, np.float32)
    osz, off = (C.c_int64 * 3)(), (C.c_double * 3)()
    assert lib.spim_psf_transformed_size(size, _model12(m), osz, off) == ERR_ARG
    assert lib.spim_transform_psf(_lib.fptr(p), size, _model12(m), _lib.fptr(out), 0) == ERR_ARG
    img, locs = pc.beads("mixed")
    idim = (C.c_int64 * 3)(*pc.IMG_DIMS)
    for lc in (locs, locs[:7]):
        orig = np.zeros((11, 9, 9), np.float32)
        st = lib.spim_extract_psf(C.c_void_p(img.ctypes.data), idim, 0, lc.ctypes.data_as(_lib._pd), len(lc), size,
                                  _model12(m), _lib.fptr(orig), _lib.fptr(out), 0)
        assert st == ERR_ARG
        with pytest.raises(_lib.SpimDeconError):
            psf.extract_psf(img, lc, pc.PSF, m)
        check_extract(img, lc, pc.PSF)                            # the mutex and the buffers are usable
    eq(psf.transform_psf(p, pc.ROT), pr.transform_psf(p, pc.ROT))


# ------------------------------------------------------------------ F. workspace reuse, batches
def test_small_psf_after_a_large_one(gpu):
    """stale dpsf / samp / dt contents beyond p.n; <= 64 and > 64 beads through one PsfWork"""
    img, locs = pc.uniform_beads(300)
    big = check_extract(img, locs, (683, 1, 3))                   # 2049 voxels, 300 beads
    small = check_extract(img, locs[:3], (3, 3, 3))
    eq(check_extract(img, locs, (683, 1, 3)), big)
    eq(check_extract(img, locs[:3], (3, 3, 3), pc.IDENT), small)
    check_extract(img, locs[:64], pc.PSF)
    check_extract(img, locs[:65], pc.PSF)


@pytest.mark.parametrize("on_device", [False, True])
def test_batch_of_different_views(gpu, on_device):
    imgs, locs, models = pc.batch_case()
    views = [torch.from_numpy(i).cuda() for i in imgs] if on_device else imgs
    got = psf.extract_psfs(views, locs, pc.PSF, models)
    for v in range(5):
        eo, et = pc.expected(imgs[v], locs[v], pc.PSF, models[v])
        eq(got[v][0], eo)
        eq(got[v][1], et)
        o, t = psf.extract_psf(views[v], locs[v], pc.PSF, models[v])
        eq(o, eo)
        eq(t, et)
    assert np.isnan(got[0][0]).all() and np.isfinite(got[4][0]).all()
    # another PSF size through the same pool, the views reversed: many beads where none were
    rev = psf.extract_psfs(views[::-1], locs[::-1], (5, 3, 17), None)
    for v in range(5):
        eq(rev[4 - v][0], pc.expected_psf(imgs[v], locs[v], (5, 3, 17)))
        assert rev[v][1] is None


def test_batch_grows_the_pool(gpu):
    imgs, locs, models = pc.batch_case()
    psf.release_workspace()
    want = [pc.expected(imgs[v], locs[v], pc.PSF, models[v]) for v in range(5)]
    for sel in ([3, 4], [0, 1, 2, 3, 4], [4]):
        got = psf.extract_psfs([imgs[v] for v in sel], [locs[v] for v in sel], pc.PSF, [models[v] for v in sel])
        for g, v in zip(got, sel):
            eq(g[0], want[v][0])
            eq(g[1], want[v][1])


def test_batch_argument_errors(gpu, lib):
    img, locs = pc.beads("mixed")
    size, idim = (C.c_int64 * 3)(*pc.PSF), (C.c_int64 * 3)(*pc.IMG_DIMS)
    orig, trans = np.zeros((11, 9, 9), np.float32), np.zeros(64 ** 3, np.float32)
    vp = C.c_void_p * 1
    one = lambda a: vp(a.ctypes.data)   # noqa: E731
    nl = (C.c_int64 * 1)(len(locs))
    # models = NULL with a transformed output
    assert lib.spim_extract_psfs(1, one(img), idim, 0, one(locs), nl, size, None, one(orig), one(trans), 0) == ERR_ARG
    assert lib.spim_extract_psfs(0, None, None, 0, None, None, size, None, None, None, 0) == 0
    assert lib.spim_extract_psfs(1, vp(None), idim, 0, one(locs), nl, size, None, one(orig), None, 0) == ERR_ARG
    assert lib.spim_extract_psfs(1, one(img), idim, 0, vp(None), nl, size, None, one(orig), None, 0) == ERR_ARG
    assert lib.spim_extract_psf(None, idim, 0, locs.ctypes.data_as(_lib._pd), len(locs), size, None, _lib.fptr(orig),
                                None, 0) == ERR_ARG
    assert lib.spim_extract_psf(C.c_void_p(img.ctypes.data), idim, 0, None, len(locs), size, None, _lib.fptr(orig),
                                None, 0) == ERR_ARG
    assert lib.spim_extract_psfs(1, one(img), idim, 0, one(locs), nl, size, None, one(orig), None, 0) == 0
    eq(orig, pc.expected_psf(img, locs, pc.PSF))


# ------------------------------------------------------------------ G. average, max projection
@pytest.mark.parametrize("shape", pc.PROJECTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_max_projection_skips_nan(gpu, shape):
    v = pc.projection_volume(shape)
    for d in (-1, 0, 1, 2):
        got, used = psf.max_projection(v, d)
        want, wused = pc.java_max_projection(v, d)
        assert used == wused
        eq(got, want)
        eq(got, pr.max_projection(v, d)[0])


def _mirror_into(p, m):
    """p[::-1, ::-1, ::-1] placed by the centre rule loc -> psfCenter - loc + avgCenter"""
    out = np.zeros(m, np.float32)
    q = p[::-1, ::-1, ::-1]
    src, dst = [], []
    for n, a in zip(p.shape, m):
        lo = n // 2 + a // 2 - (n - 1)                            # where q's index 0 lands
        src.append(slice(max(0, -lo), min(n, a - lo)))
        dst.append(slice(max(0, lo), min(a, lo + n)))
    out[tuple(dst)] = q[tuple(src)]
    return out


@pytest.mark.parametrize("shape", [(9, 7, 5), (8, 7, 5), (8, 10, 12), (1, 1, 1), (2, 1, 6)])
def test_average_of_one_psf_is_its_point_mirror(gpu, shape):
    p = _psf(shape)
    eq(psf.average_transformed_psf([p]), _mirror_into(p, shape))


def test_average_of_mixed_sizes(gpu, lib):
    """even and odd sizes per axis: an even PSF as large as the average loses its index 0"""
    ps = [_psf(s, 70 + i) for i, s in enumerate([(8, 7, 6), (7, 8, 6), (3, 8, 5), (8, 2, 1)])]
    got = psf.average_transformed_psf(ps)
    want = np.zeros((8, 8, 6), np.float32)
    for p in ps:
        want = want + _mirror_into(p, (8, 8, 6))
    eq(got, want)
    eq(got, pr.average_transformed_psf(ps))
    many = [_psf(tuple(np.random.default_rng(i).integers(1, 12, 3)), 90 + i) for i in range(17)]
    eq(psf.average_transformed_psf(many), pr.average_transformed_psf(many))
    ad = (C.c_int64 * 3)()
    dims = (C.c_int64 * 6)(6, 7, 8, 6, 8, 7)
    out = np.zeros((8, 8, 6), np.float32)
    assert lib.spim_average_transformed_psf(0, None, dims, _lib.fptr(out), ad, 0) == ERR_ARG
    ptrs = (_lib._pf * 2)(_lib.fptr(ps[0]), None)
    assert lib.spim_average_transformed_psf(2, ptrs, dims, _lib.fptr(out), ad, 0) == ERR_ARG
