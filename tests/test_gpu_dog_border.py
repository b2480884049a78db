"""GPU parity of the DoG pass in the reference's approximate GPU mode
(DifferenceOfGaussianCUDA.java:125-148: EXTEND_BORDER_PIXELS, ``extension="border"``)
against the oracle's border extension: bit-exact DoG image, exact ordered peak list."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

from oracle import dog_ref
from spim_registration_amd import _lib, dog, legacy, synthetic

pytestmark = pytest.mark.gpu

NAN = float("nan")


@functools.lru_cache(maxsize=None)
def bead_stack(shape=(40, 44, 48), cid=11):
    """The recipe of tests/test_gpu_dog.py (read-only here: shared between tests)."""
    rng = synthetic.rng_for(cid)
    t = synthetic.truth_volume(shape, rng, bead_density=1.0 / 10 ** 3)
    k = synthetic.psf(0, 1, (9, 9, 13), sigma=(1.0, 1.0, 1.6))
    from oracle import mvdecon_ref as ref
    img = ref.convolve(t.astype(np.float32), k, "mirror")
    img = (rng.poisson(np.maximum(img * 2000 + 50, 0)) + rng.normal(0, 2, shape)).astype(np.float32)
    img.setflags(write=False)
    return img


def border_dog_image(img, sigma, min_intensity=NAN, max_intensity=NAN):
    """dog_ref.process_dog:337-343 with the border extension in both Gaussians."""
    if (math.isnan(min_intensity) or math.isnan(max_intensity) or math.isinf(min_intensity)
            or math.isinf(max_intensity) or min_intensity == max_intensity):
        mn, mx = float(np.min(img)), float(np.max(img))
    else:
        mn, mx = float(np.float32(min_intensity)), float(np.float32(max_intensity))
    norm = dog_ref.normalize_image(img, mn, mx)
    s1, s2, _, kinv = dog_ref.dog_sigmas(sigma, (0.5, 0.5, 0.5))
    g1 = dog_ref.gauss3d(norm, dog_ref.cuda_kernels(s1), mode="border")
    g2 = dog_ref.gauss3d(norm, dog_ref.cuda_kernels(s2), mode="border")
    d = ((g2 - g1).astype(np.float32) * kinv).astype(np.float32)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def bead_border_dog(shape, cid, sigma, min_intensity=NAN, max_intensity=NAN):
    return border_dog_image(bead_stack(shape, cid), sigma, min_intensity, max_intensity)


def border_points(d, threshold, localization=0, find_min=False, find_max=True, ij_threads=8):
    """dog_ref.process_dog:336,344-349 over the DoG image ``d``."""
    f32 = np.float32
    min_peak = f32(threshold) if localization == 0 else f32(f32(threshold) / f32(10.0))
    peaks = dog_ref.find_peaks(d, float(min_peak), ij_threads)
    out = [(p[0], p[1], p[2], p[3]) for p in peaks if (p[5] and find_max) or (p[4] and find_min)]
    if localization == 1:
        fitted = dog_ref.quadratic_localization(d, out)
        out = [(float(x), float(y), float(z), float(v)) for x, y, z, v in fitted if abs(v) > f32(threshold)]
    return out


def assert_same(pts, d, exp, dref):
    np.testing.assert_array_equal(d, dref)
    assert [tuple(int(c) for c in p.location) for p in pts] == [e[:3] for e in exp]
    np.testing.assert_array_equal([p.intensity for p in pts], np.float32([e[3] for e in exp]))


# 1. the split z stage (default), every fused tap count
@pytest.mark.parametrize("sigma,taps,find_min", [(1.0, 7, False), (1.8, 15, False), (1.8, 15, True),
                                                 (4.0, 31, False)])
def test_border_matches_oracle_split_path(gpu, sigma, taps, find_min):
    """(40, 44, 48): one partial x strip, two y steps (the last partial), nz > K / 2.
    The border oracle differs from the mirror oracle in 30,216 / 52,220 / 80,637 of the
    84,480 voxels at these sigmas, so a mode that stayed mirror cannot pass."""
    s1, s2, _, _ = dog_ref.dog_sigmas(sigma, (0.5, 0.5, 0.5))
    assert max(len(dog_ref.cuda_kernels(s1)[0]), len(dog_ref.cuda_kernels(s2)[0])) == taps
    img = bead_stack()
    pts, d = dog.compute(img, sigma=sigma, threshold=0.008, find_min=find_min, find_max=True,
                         return_dog=True, keep_intensity=True, extension="border")
    dref = bead_border_dog((40, 44, 48), 11, sigma)
    exp = border_points(dref, 0.008, find_min=find_min)
    assert_same(pts, d, exp, dref)
    if sigma in (1.0, 1.8):
        assert len(exp) > 10
    _, dm = dog.compute(img, sigma=sigma, threshold=0.008, return_dog=True)
    assert np.count_nonzero(dm != d) > 30000   # the two modes genuinely differ


# 2. several strips, steps and z chunks
def test_border_several_strips_and_steps(gpu):
    """(150, 70, 131): two full x strips and a partial one, three y steps."""
    img = bead_stack((150, 70, 131), 21)
    pts, d = dog.compute(img, sigma=1.8, threshold=0.002, find_min=True, find_max=True, return_dog=True,
                         keep_intensity=True, extension="border")
    dref = bead_border_dog((150, 70, 131), 21, 1.8)
    exp = border_points(dref, 0.002, find_min=True)
    assert len(exp) > 5
    assert_same(pts, d, exp, dref)


def test_border_z_chunk_seams(gpu, monkeypatch):
    """16-plane chunks of k_dog_zconv over 40 planes: seams and a partial last chunk."""
    monkeypatch.setenv("SPIMDECON_DOG_ZC_CHUNK", "16")
    pts, d = dog.compute(bead_stack(), sigma=1.8, threshold=0.008, find_min=True, find_max=True, return_dog=True,
                         keep_intensity=True, extension="border")
    dref = bead_border_dog((40, 44, 48), 11, 1.8)
    assert_same(pts, d, border_points(dref, 0.008, find_min=True), dref)


# 3. the unsplit k_dog_z, scalar-index form
@pytest.mark.parametrize("sigma", [1.0, 1.8, 4.0])
def test_border_unsplit_z_stage(gpu, sigma, monkeypatch):
    monkeypatch.setenv("SPIMDECON_DOG_SPLIT", "0")
    pts, d = dog.compute(bead_stack(), sigma=sigma, threshold=0.008, find_min=True, find_max=True,
                         return_dog=True, keep_intensity=True, extension="border")
    dref = bead_border_dog((40, 44, 48), 11, sigma)
    assert_same(pts, d, border_points(dref, 0.008, find_min=True), dref)


# 4. thin volumes: the plane-table form of k_dog_z (nz <= K / 2), nx < R, ny <= R, indices
# several kernel radii outside the image
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 7), (3, 3, 3), (2, 9, 4), (5, 1, 70), (70, 3, 65), (5, 9, 70)])
def test_border_thin_volumes(gpu, shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.random(shape, dtype=np.float32)
    pts, d = dog.compute(img, sigma=1.8, threshold=0.0, find_min=True, find_max=True, return_dog=True,
                         keep_intensity=True, ij_threads=3, extension="border")
    dref = border_dog_image(img, 1.8)
    assert_same(pts, d, border_points(dref, 0.0, find_min=True, ij_threads=3), dref)


# 5. the 63-tap fallback (csrc/sepconv.hip: sep_pass with the border mode)
def test_border_63_tap_fallback(gpu):
    s1, s2, _, _ = dog_ref.dog_sigmas(8.0, (0.5, 0.5, 0.5))
    assert len(dog_ref.cuda_kernels(s2)[0]) == 63
    pts, d = dog.compute(bead_stack(), sigma=8.0, threshold=0.002, find_min=True, find_max=True, return_dog=True,
                         keep_intensity=True, extension="border")
    dref = bead_border_dog((40, 44, 48), 11, 8.0)
    assert_same(pts, d, border_points(dref, 0.002, find_min=True), dref)


# 6. a caller-given intensity range (no tap trim: mm[2] = 1), and the trim on / off pair
def test_border_given_intensity_range(gpu):
    img = bead_stack((24, 26, 30), 12)
    pts, d = dog.compute(img, sigma=2.0, threshold=0.004, min_intensity=0.0, max_intensity=4000.0,
                         return_dog=True, keep_intensity=True, extension="border")
    dref = bead_border_dog((24, 26, 30), 12, 2.0, 0.0, 4000.0)
    assert_same(pts, d, border_points(dref, 0.004), dref)


def test_border_zero_tap_trim_bit_identical(gpu, monkeypatch):
    out = {}
    for t in ("1", "0"):
        monkeypatch.setenv("SPIMDECON_DOG_TRIM", t)
        pk, d = dog.compute(bead_stack(), sigma=1.8, threshold=1e-4, find_min=True, find_max=True,
                            return_dog=True, keep_intensity=True, extension="border")
        out[t] = ([(tuple(p.location), p.intensity) for p in pk], d)
    np.testing.assert_array_equal(out["1"][1], out["0"][1])
    assert out["1"][0] == out["0"][0] and len(out["1"][0]) > 10
    np.testing.assert_array_equal(out["1"][1], bead_border_dog((40, 44, 48), 11, 1.8))


# 7. localization 1 over the border DoG
@pytest.mark.parametrize("find_min,find_max", [(False, True), (True, True)])
def test_border_quadratic_localization(gpu, find_min, find_max):
    img = bead_stack((40, 44, 48), 13)
    pts, d = dog.compute(img, sigma=1.8, threshold=0.008, localization=1, find_min=find_min, find_max=find_max,
                         return_dog=True, keep_intensity=True, extension="border")
    dref = bead_border_dog((40, 44, 48), 13, 1.8)
    exp = border_points(dref, 0.008, localization=1, find_min=find_min, find_max=find_max)
    np.testing.assert_array_equal(d, dref)
    assert len(pts) == len(exp) and len(exp) > 10
    got = np.array([p.location for p in pts])
    want = np.array([e[:3] for e in exp])
    # identical double arithmetic; float32-rounded positions
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
    np.testing.assert_allclose([p.intensity for p in pts], [e[3] for e in exp], rtol=1e-6, atol=1e-9)
    assert np.any(np.abs(got - np.round(got)) > 1e-3)      # genuinely sub-pixel


# 8. GPU-tensor input, tensor DoG output, the array API and the peak API
def test_border_device_tensor_route(gpu):
    img = bead_stack((24, 26, 30), 13)
    pts, d = dog.compute(img, localization=1, return_dog=True, keep_intensity=True, extension="border")
    np.testing.assert_array_equal(d, bead_border_dog((24, 26, 30), 13, 1.8))
    dimg = torch.from_numpy(img.copy()).to("cuda:0")
    tpts, td = dog.compute(dimg, localization=1, return_dog=True, keep_intensity=True, extension="border")
    assert td.is_cuda
    np.testing.assert_array_equal(td.cpu().numpy(), d)
    assert len(pts) > 0
    assert [(p.location, p.intensity) for p in tpts] == [(p.location, p.intensity) for p in pts]
    pos, inten = dog.interest_points_array(dimg, localization=1, extension="border")
    np.testing.assert_array_equal(pos, np.array([p.location for p in pts]).reshape(-1, 3))
    np.testing.assert_array_equal(inten, np.float32([p.intensity for p in pts]))
    pk = dog.simple_peaks(img, threshold=0.008, localization=0, find_min=True, find_max=True, extension="border")
    e = dog_ref.find_peaks(np.asarray(d), float(np.float32(0.008)))
    assert [q[:3] for q in pk] == [q[:3] for q in e] and [q[4:] for q in pk] == [q[4:] for q in e]


# 9. the mirror mode is what it was; bad modes are refused
def test_mirror_extension_is_the_default(gpu):
    img = bead_stack()
    a, da = dog.compute(img, sigma=1.8, threshold=0.008, return_dog=True, keep_intensity=True)
    b, db = dog.compute(img, sigma=1.8, threshold=0.008, return_dog=True, keep_intensity=True, extension="mirror")
    np.testing.assert_array_equal(da, db)
    assert [(p.location, p.intensity) for p in a] == [(p.location, p.intensity) for p in b]
    exp, dref = dog_ref.process_dog(img, 1.8, 0.008)
    assert_same(b, db, exp, dref)


def test_bad_extension_is_refused(gpu):
    img = np.ascontiguousarray(bead_stack((24, 26, 30), 12))
    for bad in ("clamp", "", None, 1):
        with pytest.raises(ValueError, match="extension"):
            dog.compute(img, extension=bad)
    with pytest.raises(ValueError, match="extension"):
        dog.simple_peaks(img, extension="clamp")
    lib = _lib.load()
    p = _lib.DogParams()
    lib.spim_dog_params_default(C.byref(p))
    dims = (C.c_int64 * 3)(img.shape[2], img.shape[1], img.shape[0])
    n = C.c_int64(-1)
    for ext in (2, -1):
        st = lib.spim_dog_compute_ext(_lib.fptr(img), dims, C.byref(p), ext, None, None, 0, C.byref(n))
        assert st == -1 and "extension" in _lib.last_error()    # SPIMDECON_ERR_ARG
        st = lib.spim_dog_interest_points_ext(_lib.fptr(img), dims, C.byref(p), ext, None, None, 0, C.byref(n))
        assert st == -1 and "extension" in _lib.last_error()
    assert n.value == -1
    assert lib.spim_dog_compute_ext(_lib.fptr(img), dims, C.byref(p), 1, None, None, 0, C.byref(n)) == 0
    assert n.value >= 0


# 10. the reference's own procedure (blocks through convolve_N with OOB 2) against the fused mode
def test_reference_block_procedure_equals_fused_border(gpu):
    """DifferenceOfGaussianCUDA's approximate branch restated (legacy.gauss_blocks_cuda) with
    2 x 2 x 3 blocks and as one block, through the separately tested convolve_N: both equal
    the fused ``extension="border"`` DoG bit for bit -- independent of the oracle's
    convolution."""
    img = bead_stack((36, 40, 48), 15)
    norm = dog_ref.normalize_image(img, float(img.min()), float(img.max()))
    assert norm.min() == 0.0 and norm.max() == 1.0     # the fused pass's own normalisation is the identity
    s1, s2, _, kinv = dog_ref.dog_sigmas(1.8, (0.5, 0.5, 0.5))
    _, fused = dog.compute(norm, sigma=1.8, return_dog=True, extension="border")
    cuda = legacy.CUDASeparableConvolution()
    for nb in ((2, 2, 3), (1, 1, 1)):
        g1 = legacy.gauss_blocks_cuda(norm, s1, nb, False, cuda, 0)
        g2 = legacy.gauss_blocks_cuda(norm, s2, nb, False, cuda, 0)
        np.testing.assert_array_equal(((g2 - g1).astype(np.float32) * kinv).astype(np.float32), fused)
