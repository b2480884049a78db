"""CPU: the asymmetric PSF fixture (synthetic.psf_asymmetric) is non-degenerate, and the
oracle's RL loop is sensitive to the kernel orientation with it.

``synthetic.psf`` is a centred Gaussian rotated about y: centro-symmetric for every view,
mirror-symmetric in y, and for V = 2 (0 and 90 degrees) mirror-symmetric in x and z too.
With such kernels ``inverted_kernel`` is the identity, the kernel spectrum is real and a
kernel equals its flips, so an orientation or conjugation mistake anywhere on the
convolution path moves nothing.  tests/test_gpu_asym_psf.py runs the HIP paths with the
kernels checked here; this file shows that those kernels have none of the symmetries
(conditions on the inputs, not tolerances) and that the f64 oracle, the yardstick of
those tests, moves by 200 times their 1e-4 bound when a kernel is mis-oriented.
"""
import numpy as np
import pytest

from conftest import rel_l2
from oracle import mvdecon_ref as ref
from spim_registration_amd import synthetic

# the Gaussian tails of a 31-point grid underflow float32 at the default sigma (so do
# synthetic.psf's); the large compound-kernel cases use a wider Gaussian to keep every
# tap positive
BIG_SIGMA = (3.0, 3.0, 7.0)
BIG_SIZES = ((31, 19, 31), (25, 19, 21))


def asym_psf(view, num_views, size):
    """The asymmetric kernel of (view, num_views, size) as every test here and in
    test_gpu_asym_psf.py uses it."""
    if tuple(size) in BIG_SIZES:
        return synthetic.psf_asymmetric(view, num_views, size, sigma=BIG_SIGMA)
    return synthetic.psf_asymmetric(view, num_views, size)


# (num_views, ksize) of every kernel set the GPU tests and the golden fixtures use (the sets
# with one size per view, and the 4- and 6-view ones: tests/test_rl_long_cpu.py)
PSF_SETS = [
    (3, (7, 9, 11)), (3, (9, 7, 11)), (3, (5, 9, 7)),        # kernel preparation, whole RL, lrsim
    (4, (31, 19, 31)), (4, (25, 19, 21)),                    # block-parallel compound kernels
    (3, (9, 7, 5)), (3, (5, 5, 9)),                          # y split, lrsim
    (2, (5, 7, 9)), (3, (5, 5, 7)),                          # golden fixtures, z slabs
    (2, (9, 7, 9)),                                          # device groups
    (2, (9, 5, 7)), (2, (3, 3, 25)), (2, (3, 3, 31)), (2, (3, 3, 23)), (2, (5, 5, 3)),   # z passes
    (2, (9, 9, 9)), (2, (21, 3, 3)), (2, (25, 5, 3)),        # x tiles
    (2, (3, 25, 3)),                                         # y passes
    (2, (5, 7, 3)),                                          # Stockham passes
]
PSF_CASES = [(v, V, size) for V, size in PSF_SETS for v in range(V)]


def imag_ratio(k):
    """max |Im K^| / max |K^| of the kernel zero-padded to 32^3, centre at the origin."""
    kp = np.zeros((32, 32, 32))
    kz, ky, kx = k.shape
    kp[:kz, :ky, :kx] = k
    kp = np.roll(kp, (-(kz // 2), -(ky // 2), -(kx // 2)), (0, 1, 2))
    f = np.fft.fftn(kp)
    return float(np.abs(f.imag).max() / np.abs(f).max())


@pytest.mark.parametrize("view,num_views,size", PSF_CASES)
def test_asymmetric_psf_is_non_degenerate(view, num_views, size):
    k = asym_psf(view, num_views, size)
    assert k.dtype == np.float32 and k.shape == size[::-1]
    assert abs(float(k.astype(np.float64).sum()) - 1.0) < 1e-6
    assert (k > 0).all()
    assert rel_l2(ref.inverted_kernel(k), k) >= 0.3
    for ax in range(3):
        if k.shape[ax] > 1:
            assert rel_l2(np.flip(k, ax), k) >= 0.1, ax
    assert imag_ratio(k) >= 0.05


def test_symmetric_psf_is_degenerate():
    """Why the fixture exists: synthetic.psf has every symmetry, exactly."""
    for V, size in PSF_SETS:
        for v in range(V):
            k = synthetic.psf(v, V, size)
            assert np.array_equal(ref.inverted_kernel(k), k)
            assert np.array_equal(np.flip(k, 1), k)
            assert imag_ratio(k) < 1e-12
            if V == 2:
                assert np.array_equal(np.flip(k, 0), k) and np.array_equal(np.flip(k, 2), k)


SHAPE, V, KSIZE, ITERS, LAM = (20, 24, 28), 3, (7, 9, 11), 5, 0.006

FAULTS = {
    "k2_inverted_again": lambda k1, k2: (k1, [ref.inverted_kernel(k) for k in k2]),
    "k2_flipped_in_y": lambda k1, k2: (k1, [np.flip(k, 1).copy() for k in k2]),
    "k1_flipped_in_z": lambda k1, k2: ([np.flip(k, 0).copy() for k in k1], k2),
    "k1_flipped_in_x": lambda k1, k2: ([np.flip(k, 2).copy() for k in k1], k2),
}


def _rl(imgs, ws, k1, k2):
    _, avg = ref.first_iteration(imgs)
    psi = np.full(SHAPE, np.float32(avg), np.float32)
    for _ in range(ITERS):
        psi, _ = ref.run_iteration(psi, imgs, ws, k1, k2, LAM)
    return psi


@pytest.fixture(scope="module", params=[True, False], ids=["asymmetric", "symmetric"])
def views(request):
    imgs, ws, ks, _ = synthetic.make_views(SHAPE, V, config_id=7, ksize=KSIZE, weights="blend",
                                           bead_density=1.0 / 6 ** 3, asymmetric=request.param)
    return request.param, imgs, ws, ks


@pytest.mark.parametrize("psftype", list(ref.PSFTYPE))
def test_oracle_is_sensitive_to_kernel_orientation(views, psftype):
    """Each fault moves the oracle's psi by rel-L2 >= 1e-2 with asymmetric kernels
    (measured 2e-2 .. 1.3e-1), 100 times the GPU tests' 1e-4 bound.  With synthetic.psf
    re-inverting K2 or flipping it in y moves psi by exactly 0: the gap the asymmetric
    tests close."""
    asym, imgs, ws, ks = views
    k1, k2 = ref.prepare_kernels(ks, psftype, 8)
    psi = _rl(imgs, ws, k1, k2)
    assert np.isfinite(psi).all()
    for name, fault in FAULTS.items():
        f1, f2 = fault(k1, k2)
        moved = rel_l2(_rl(imgs, ws, f1, f2), psi)
        print(f"{'asym' if asym else 'sym'} {psftype.name} {name}: {moved:.3e}")
        if asym:
            assert moved >= 1e-2, (name, moved)
        elif name.startswith("k2"):
            assert moved == 0.0, (name, moved)
