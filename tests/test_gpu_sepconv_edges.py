"""The separable convolution passes of csrc/sepconv.hip at their edges: every tap count of
the convolve_N ABI, the seams of every tiled kernel, every dispatch route of sep_pass, and
the DoG routes that go through them -- bit for bit against the plain reference of
tests/sepconv_cases.py (float32, tap order, every tap visited; its premises:
tests/test_sepconv_premises_cpu.py) or, for the DoG, against oracle/dog_ref.py.

Where each instantiation runs (shapes (nz, ny, nx)):
  k_sep_x<1>, several blocks     test_every_tap_count_and_mode (nx 257, ny 9), test_kernel_seams
                                 (nx 255 .. 513 with ny 8 and 17)
  k_sep_yz<1, 1|2, 7|15>         test_every_tap_count_and_mode at 7 and 15 taps (two z tiles, the
                                 cut inside a thread's 16 outputs), test_kernel_seams at 15 taps
                                 (63 .. 129 along y and z, nx 63 .. 65)
  k_sep_yz<1, 1|2, 0>            the same two at 31, 63 and 127 taps
  k_sep_yz<2, 2, 7|15|0>         test_unfused_dog_tall_volume (sigma 1.0, 1.8, 8.0), writing the DoG
  k_sep_yz<2, 1, 15>             test_unfused_dog_long_rows
  k_sep_yz<2, 1|2, 0> at 127     test_dog_127_taps (the largest LDS request, 98,296 bytes)
  k_sep_pass<1>                  test_grid_stride_fallback (x, y and z passes)
  k_sep_pass<2>                  test_unfused_dog_tall_volume (x with the on-the-fly normalisation,
                                 y), test_unfused_dog_long_rows (x, and z writing the DoG)
  31 taps                        convolve_31 in test_every_tap_count_and_mode, test_kernel_seams,
                                 test_gauss_2d_and_1d_images
  127 taps                       convolve_127 in test_every_tap_count_and_mode,
                                 test_axes_shorter_than_the_reach; the DoG in test_dog_127_taps
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import sepconv_cases as sc
from oracle import dog_ref
from spim_registration_amd import _lib, dog, legacy
from test_gpu_dog_border import border_dog_image, border_points

pytestmark = pytest.mark.gpu


def convolve(K, img, ks, mode, on=(True, True, True), value=sc.OOB_VALUE):
    """convolve_K on a copy of ``img`` [z, y, x]; a switched-off axis gets a null kernel.
    Returns (the ABI's boolean, the image afterwards)."""
    nz, ny, nx = img.shape
    im = np.array(img, np.float32, order="C").reshape(-1)
    kk = [k if o else None for k, o in zip(ks, on)]
    ok = legacy.CUDASeparableConvolution()._conv(K, im, kk[0], kk[1], kk[2], nx, ny, nz, on[0], on[1], on[2],
                                                 int(mode), value, 0)
    return ok, im.reshape(img.shape)


# ------------------------------------------------------------------ a.
@pytest.mark.parametrize("K,mode", sc.ALL_TAPS_CASES)
def test_every_tap_count_and_mode(gpu, K, mode):
    """convolve_{7, 15, 31, 63, 127} x the four modes on (70, 9, 257): two x blocks (the
    last one column), two row groups (the last one row), two z tiles (the last 6 planes,
    cut inside one thread's run of 16 outputs), asymmetric taps different per axis.
    k_sep_x<1>; k_sep_yz<1, 1|2, 7|15> (window) and <1, 1|2, 0> (loop; 127 taps: the
    first run of its 49,148-byte LDS request)."""
    img = sc.volume(sc.ALL_TAPS_SHAPE, sc.ALL_TAPS_SEED)
    ok, out = convolve(K, img, sc.random_taps(K, sc.all_taps_seed(K)), mode)
    assert ok is True, _lib.last_error()
    np.testing.assert_array_equal(out, sc.expected(sc.ALL_TAPS_SHAPE, sc.ALL_TAPS_SEED, K, sc.all_taps_seed(K), mode))


# ------------------------------------------------------------------ b.
@pytest.mark.parametrize("K", sc.SEAM_TAPS)
@pytest.mark.parametrize("mode", sc.SEAM_MODES)
@pytest.mark.parametrize("shape", sc.SEAM_SHAPES)
def test_kernel_seams(gpu, shape, mode, K):
    """One short of, exactly, one past and twice past each tile: nx 255 .. 513 over the
    256-column blocks of k_sep_x<1> with ny 8 and 17 (8-row groups); 63 .. 129 along y and
    z over the 64-position tiles of k_sep_yz<1, 1|2, 15> (window) and <1, 1|2, 0> (31
    taps, loop), nx 63 .. 65 over their 64-column tiles (sepconv_cases.SEAM_SHAPES)."""
    img = sc.volume(shape, sc.SEAM_SEED)
    ok, out = convolve(K, img, sc.random_taps(K, sc.SEAM_SEED + K), mode)
    assert ok is True, _lib.last_error()
    np.testing.assert_array_equal(out, sc.expected(shape, sc.SEAM_SEED, K, sc.SEAM_SEED + K, mode))


# ------------------------------------------------------------------ c.
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("shape,K", sc.SHORT_CASES)
def test_axes_shorter_than_the_reach(gpu, shape, K, mode):
    """(1, 2, 300) at 127 taps, (2, 1, 3) at 63, (1, 1, 1) at 7: axes of 1, 2 and 3
    samples under a reach of up to 63 (mirror folds many times; n == 1 reads index 0)."""
    img = sc.volume(shape, sc.SHORT_SEED)
    ok, out = convolve(K, img, sc.random_taps(K, sc.SHORT_SEED + K), mode)
    assert ok is True, _lib.last_error()
    np.testing.assert_array_equal(out, sc.expected(shape, sc.SHORT_SEED, K, sc.SHORT_SEED + K, mode))


# ------------------------------------------------------------------ d.
@pytest.mark.parametrize("on", sc.SWITCHES)
def test_axis_switches(gpu, on):
    """convolveX/Y/Z: each single axis, each pair, none (the image comes back unchanged);
    the kernel of a switched-off axis is a null pointer."""
    K = sc.SWITCH_TAPS
    img = sc.volume(sc.SWITCH_SHAPE, sc.SWITCH_SEED)
    for mode in (sc.VALUE, sc.MIRROR):
        ok, out = convolve(K, img, sc.random_taps(K, sc.SWITCH_TAP_SEED), mode, on)
        assert ok is True, _lib.last_error()
        exp = sc.expected(sc.SWITCH_SHAPE, sc.SWITCH_SEED, K, sc.SWITCH_TAP_SEED, mode, on)
        np.testing.assert_array_equal(out, exp)
        if not any(on):
            np.testing.assert_array_equal(out, img)
        else:
            assert np.mean(out != sc.expected(sc.SWITCH_SHAPE, sc.SWITCH_SEED, K, sc.SWITCH_TAP_SEED, mode)) > 0.99


def test_bad_arguments_return_false_and_leave_the_image(gpu):
    """A switched-on axis with a null kernel, and a mode outside 0 .. 3."""
    K = sc.SWITCH_TAPS
    img = sc.volume(sc.SWITCH_SHAPE, sc.SWITCH_SEED)
    ks = sc.random_taps(K, sc.SWITCH_TAP_SEED)
    nz, ny, nx = img.shape
    cuda = legacy.CUDASeparableConvolution()
    for missing in range(3):
        kk = [None if a == missing else k for a, k in enumerate(ks)]
        im = img.copy().reshape(-1)
        assert cuda._conv(K, im, kk[0], kk[1], kk[2], nx, ny, nz, True, True, True, sc.BORDER, 0.0, 0) is False
        assert "null kernel" in _lib.last_error()
        np.testing.assert_array_equal(im.reshape(img.shape), img)
    for mode in (4, -1):
        ok, out = convolve(K, img, ks, mode)
        assert ok is False and "outofbounds" in _lib.last_error()
        np.testing.assert_array_equal(out, img)
    ok, out = convolve(K, img, ks, sc.BORDER)          # and the next call is served
    assert ok is True
    np.testing.assert_array_equal(out, sc.expected(sc.SWITCH_SHAPE, sc.SWITCH_SEED, K, sc.SWITCH_TAP_SEED, sc.BORDER))


@pytest.mark.parametrize("mode", sc.MODES)
def test_gauss_2d_and_1d_images(gpu, mode):
    """legacy.gauss with dim = [300, 70] (d = 1, z off, 31 taps) and dim = [300] (h = d = 1,
    y and z off, 15 taps): Gaussian taps, the missing axes switched off with null kernels."""
    cuda = legacy.CUDASeparableConvolution()
    for dim, sigma, K in ((sc.GAUSS_2D_DIM, sc.GAUSS_2D_SIGMA, 31), (sc.GAUSS_1D_DIM, sc.GAUSS_1D_SIGMA, 15)):
        shape = (1, dim[1] if len(dim) > 1 else 1, dim[0])
        img = sc.volume(shape, sc.GAUSS_SEED)
        ks = legacy.get_cuda_kernels(sigma)
        assert len(ks[0]) == K
        im = img.copy().reshape(-1)
        assert legacy.gauss(im, dim, sigma, legacy.OutOfBounds(mode), sc.OOB_VALUE, cuda, 0) is True
        on = tuple(a < len(dim) for a in range(3))
        exp = sc.ref3d(img, list(ks) + [None] * (3 - len(ks)), mode, sc.OOB_VALUE, on)
        np.testing.assert_array_equal(im.reshape(shape), exp)


# ------------------------------------------------------------------ e.
@pytest.mark.parametrize("K", sc.FALLBACK_TAPS)
@pytest.mark.parametrize("mode", sc.FALLBACK_MODES)
@pytest.mark.parametrize("whd", sc.FALLBACK_WHD)
def test_grid_stride_fallback(gpu, whd, mode, K):
    """k_sep_pass<1>, the 64-bit-index grid-stride kernel, with 131,072 voxels: a grid
    extent past 65535 sends a pass there.  (w, h, d) = (2, 1, 65536): the x and y passes
    (z stays tiled, 1,024 tiles along z); (1, 65536, 2): the x and z passes."""
    w, h, d = whd
    img = sc.volume((d, h, w), sc.FALLBACK_SEED)
    ok, out = convolve(K, img, sc.random_taps(K, sc.FALLBACK_SEED + K), mode)
    assert ok is True, _lib.last_error()
    np.testing.assert_array_equal(out, sc.expected((d, h, w), sc.FALLBACK_SEED, K, sc.FALLBACK_SEED + K, mode))


# ------------------------------------------------------------------ f.
def noise(shape, seed):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def run_dog(img, sigma, extension="mirror"):
    return dog.compute(img, sigma=sigma, threshold=0.0, find_min=True, find_max=True, return_dog=True,
                       keep_intensity=True, ij_threads=3, extension=extension)


def assert_dog(pts, d, exp, dref):
    np.testing.assert_array_equal(d, dref)
    assert [tuple(int(c) for c in p.location) for p in pts] == [e[:3] for e in exp]
    np.testing.assert_array_equal([p.intensity for p in pts], np.float32([e[3] for e in exp]))


@pytest.mark.parametrize("sigma,K", sc.DOG_TALL_SIGMAS)
def test_unfused_dog_tall_volume(gpu, sigma, K):
    """(65536, 3, 3): nz > 65535 keeps a 7-, 15- or 63-tap DoG off the fused kernels.  x and
    y passes: k_sep_pass<2> (x with the on-the-fly normalisation); z: k_sep_yz<2, 2, 7>,
    <2, 2, 15> (register window) or <2, 2, 0> (63 taps), over 1,024 z tiles, writing
    (g2 - g1) * scale.  Uniform noise, threshold 0, both extrema."""
    assert sc.dog_taps(sigma) == K
    img = noise(sc.DOG_TALL_SHAPE, sc.DOG_TALL_SEED)
    pts, d = run_dog(img, sigma)
    exp, dref = dog_ref.process_dog(img, sigma, 0.0, find_min=True, find_max=True, ij_threads=3)
    assert len(exp) > 10
    assert_dog(pts, d, exp, dref)


def test_unfused_dog_tall_volume_border(gpu):
    """The same route with extension="border" at 15 taps."""
    img = noise(sc.DOG_TALL_SHAPE, sc.DOG_TALL_SEED)
    pts, d = run_dog(img, 1.8, "border")
    dref = border_dog_image(img, 1.8)
    exp = border_points(dref, 0.0, find_min=True, ij_threads=3)
    assert len(exp) > 10
    assert_dog(pts, d, exp, dref)
    assert np.mean(d != dog_ref.process_dog(img, 1.8, 0.0)[1]) > 0.5    # (not the mirror image)


def test_unfused_dog_long_rows(gpu):
    """(1, 2097121, 1): ny > 65535 * 32 keeps the 15-tap DoG off the fused kernels.  y pass:
    k_sep_yz<2, 1, 15> over 32,768 y tiles; x pass and the DoG-writing z pass:
    k_sep_pass<2> (grid extent ny).  No voxel has 26 neighbours: an empty peak list."""
    img = noise(sc.DOG_LONG_SHAPE, sc.DOG_LONG_SEED)
    pts, d = run_dog(img, 1.8)
    exp, dref = dog_ref.process_dog(img, 1.8, 0.0, find_min=True, find_max=True, ij_threads=3)
    np.testing.assert_array_equal(d, dref)
    assert pts == [] and exp == []


# ------------------------------------------------------------------ g.
@pytest.mark.parametrize("extension", ["mirror", "border"])
def test_dog_127_taps(gpu, extension):
    """sigma 12 on (70, 20, 150): 127 taps, k_sep_x<2> and k_sep_yz<2, 1|2, 0> with the
    file's largest LDS request (2 x 190 x 64 operand pairs + taps = 98,296 bytes, above the
    64 KiB a kernel gets without hipFuncSetAttribute); two z tiles, three x tiles."""
    s1, s2, _, _ = dog_ref.dog_sigmas(sc.DOG_127_SIGMA, (0.5, 0.5, 0.5))
    assert len(dog_ref.cuda_kernels(s2)[0]) == 127 and sc.dog_taps(sc.DOG_127_SIGMA) == 127
    img = noise(sc.DOG_127_SHAPE, sc.DOG_127_SEED)
    pts, d = run_dog(img, sc.DOG_127_SIGMA, extension)
    if extension == "mirror":
        exp, dref = dog_ref.process_dog(img, sc.DOG_127_SIGMA, 0.0, find_min=True, find_max=True, ij_threads=3)
    else:
        dref = border_dog_image(img, sc.DOG_127_SIGMA)
        exp = border_points(dref, 0.0, find_min=True, ij_threads=3)
    assert len(exp) > 10
    assert_dog(pts, d, exp, dref)


def test_dog_sigma_18_is_refused_and_the_workspace_survives(gpu):
    """Gaussians longer than 127 taps are refused (an argument error naming the limit) by
    both entry points, and the detector workspace serves the next call with the same bits,
    on the fused route and on the separate passes."""
    assert sc.dog_taps(sc.DOG_REFUSED_SIGMA) is None
    img = noise((24, 26, 30), 811)
    before = [run_dog(img, s) for s in (1.8, 8.0)]
    for call in (lambda: dog.compute(img, sigma=sc.DOG_REFUSED_SIGMA),
                 lambda: dog.simple_peaks(img, sigma=sc.DOG_REFUSED_SIGMA)):
        with pytest.raises((ValueError, _lib.SpimDeconError), match="127") as e:
            call()
        if isinstance(e.value, _lib.SpimDeconError):
            assert e.value.status == -1      # SPIMDECON_ERR_ARG
    lib = _lib.load()
    p = _lib.DogParams()
    lib.spim_dog_params_default(C.byref(p))
    p.sigma = sc.DOG_REFUSED_SIGMA
    dims = (C.c_int64 * 3)(30, 26, 24)
    n = C.c_int64(-1)
    assert lib.spim_dog_compute_ext(_lib.fptr(img), dims, C.byref(p), 0, None, None, 0, C.byref(n)) == -1
    assert "127" in _lib.last_error() and n.value == -1
    for (pts0, d0), s in zip(before, (1.8, 8.0)):
        pts, d = run_dog(img, s)
        np.testing.assert_array_equal(d, d0)
        assert [(q.location, q.intensity) for q in pts] == [(q.location, q.intensity) for q in pts0]
        np.testing.assert_array_equal(d, dog_ref.process_dog(img, s, 0.0)[1])


# ------------------------------------------------------------------ h.
@pytest.mark.parametrize("mode", [sc.ZERO, sc.MIRROR])
def test_non_finite_input_spreads_over_the_padded_footprint(gpu, mode):
    """convolve_15 with Gaussians of 7, 11 and 9 taps padded to 15: the kernels multiply
    the zero taps too (0 * NaN = 0 * inf = NaN), so one NaN and one +inf turn the whole
    15^3 footprint into NaN -- more than the zero-skipping oracle (dog_ref.convolve_axis)
    predicts.  Records the behaviour of convolve_N as it is."""
    ks = legacy.get_cuda_kernels(sc.NONFINITE_SIGMAS)
    assert len(ks[0]) == 15
    img = sc.nonfinite_volume()
    ok, out = convolve(15, img, ks, mode)
    assert ok is True, _lib.last_error()
    exp = sc.ref3d(img, ks, mode, sc.OOB_VALUE)
    np.testing.assert_array_equal(np.isnan(out), np.isnan(exp))
    np.testing.assert_array_equal(out, exp)
    with np.errstate(invalid="ignore"):
        skip = dog_ref.gauss3d(img, ks, sc.MODE_NAMES[mode], sc.OOB_VALUE)
    assert np.isnan(out).sum() > np.isnan(skip).sum() > 0


# ------------------------------------------------------------------ i.
@pytest.mark.parametrize("K", sc.TAP_COUNTS)
def test_single_pass_within_the_float64_bound(gpu, K):
    """One x pass and one z pass of the (70, 9, 257) volume against the float64 sum:
    |out - out64| <= gamma_(K + 1) * sum |v k| (sepconv_cases.pass_bound, derived from the
    K products and additions in float32) -- the anchor of the bit-exact reference."""
    img = sc.volume(sc.ALL_TAPS_SHAPE, sc.ALL_TAPS_SEED)
    ks = sc.random_taps(K, sc.all_taps_seed(K))
    for axis in (0, 2):
        on = tuple(a == axis for a in range(3))
        ok, out = convolve(K, img, ks, sc.MIRROR, on)
        assert ok is True, _lib.last_error()
        o64, mag = sc.ref_pass64(img, ks[axis], axis, sc.MIRROR)
        err = np.abs(out.astype(np.float64) - o64)
        assert np.all(err <= sc.pass_bound(K, mag)), float((err / mag).max())
        assert err.max() > 0      # (float32 arithmetic: the comparison is not vacuous)
