"""The detectors and the downsampler (csrc/dog.hip, dom.hip, downsample.hip) share one call
scaffold and one persistent, grow-only workspace per device (csrc/detect.hpp): a call must not
depend on what ran before it.  One process, one device, one fixed order of calls in which each
finds buffers left by a different detector and of a different size; every result equal to what
the per-detector tests compare against (oracle/dog_ref.py, tests/dom_ref.py,
tests/downsample_ref.py), compared as tests/test_gpu_{dog,dog_border,dom,downsample}.py compare:
the images bit for bit, the ordered points exactly, fitted positions as
test_dog_quadratic_localization."""
import functools

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import dom_ref
import downsample_ref
from oracle import dog_ref
from spim_registration_amd import _lib, dog, dom, downsample
from test_gpu_dog_border import bead_stack, border_dog_image, border_points
from test_gpu_dom import same_bits
from test_gpu_downsample import volume

pytestmark = pytest.mark.gpu

LARGEST = ((40, 44, 48), 13)     # the bead stack of the border tests: the largest view here
DOM_VIEW = ((24, 26, 30), 12)
# nz = 3 at 7 taps (nz <= K / 2): the shape class the default configuration sends through the
# unsplit, table-indexed k_dog_z; 70 x 20 columns are two boxes along x and three along y
THIN = (3, 20, 70)


@functools.lru_cache(maxsize=None)
def largest_dog():
    return dog_ref.process_dog(bead_stack(*LARGEST), 1.8, 0.008, localization=1, find_min=True, find_max=True)


def check_largest_dog():
    pts, d = dog.compute(bead_stack(*LARGEST), sigma=1.8, threshold=0.008, localization=1, find_min=True,
                         find_max=True, return_dog=True, keep_intensity=True)
    exp, dref = largest_dog()
    np.testing.assert_array_equal(d, dref)
    assert len(pts) == len(exp) and len(exp) > 10
    np.testing.assert_allclose(np.array([p.location for p in pts]), np.array([e[:3] for e in exp]), rtol=0, atol=1e-5)
    np.testing.assert_allclose([p.intensity for p in pts], [e[3] for e in exp], rtol=1e-6, atol=1e-9)


def check_points(pts, exp):
    assert [tuple(int(c) for c in p.location) for p in pts] == [e[:3] for e in exp]
    np.testing.assert_array_equal(np.float32([p.intensity for p in pts]), np.float32([e[3] for e in exp]))


def test_calls_do_not_depend_on_the_calls_before(gpu, lib):
    # 1: downsample from a host array (w.in, w.tmp_a, w.dog)
    v1 = volume((24, 40, 72), seed=1)
    same_bits(downsample.downsample(v1, 2, 2), downsample_ref.downsample(v1, 2, 2))
    # 2: DoG mirror with quadratic localisation on the largest view: every buffer grows
    check_largest_dog()
    # 3: DoM on a smaller view, stale tails in every buffer
    v3 = bead_stack(*DOM_VIEW)
    exp3, _, dom3 = dom_ref.process_dom(np.asarray(v3), threshold=0.0025, find_min=True, find_max=True)
    pts, d = dom.compute(v3, threshold=0.0025, find_min=True, find_max=True, return_dom=True, keep_intensity=True)
    same_bits(d, dom3)
    assert len(exp3) > 10
    check_points(pts, exp3)
    # 4: DoG border on the smallest view
    v4 = np.random.default_rng(4).random(THIN, dtype=np.float32)
    s1, s2, _, _ = dog_ref.dog_sigmas(1.0, (0.5, 0.5, 0.5))
    assert max(len(dog_ref.cuda_kernels(s1)[0]), len(dog_ref.cuda_kernels(s2)[0])) == 7
    pts, d = dog.compute(v4, sigma=1.0, threshold=0.0, find_min=True, find_max=True, return_dog=True,
                         keep_intensity=True, ij_threads=3, extension="border")
    dog4 = border_dog_image(v4, 1.0)
    exp4 = border_points(dog4, 0.0, find_min=True, ij_threads=3)
    np.testing.assert_array_equal(d, dog4)
    assert len(exp4) > 10
    check_points(pts, exp4)
    # 5: downsample into a device tensor
    v5 = volume((33, 37, 50), seed=5)
    out = downsample.downsample(torch.from_numpy(v5).cuda(), 4, 1)
    assert out.is_cuda
    same_bits(out.cpu().numpy(), downsample_ref.downsample(v5, 4, 1))
    # 6: DoG through the separable fallback (63 taps; smoothed noise at threshold 0 has an extremum)
    v6 = np.random.default_rng(6).random((30, 34, 40), dtype=np.float32)
    s1, s2, _, _ = dog_ref.dog_sigmas(8.0, (0.5, 0.5, 0.5))
    assert len(dog_ref.cuda_kernels(s2)[0]) == 63
    pts, d = dog.compute(v6, sigma=8.0, threshold=0.0, find_min=True, find_max=True, return_dog=True,
                         keep_intensity=True)
    exp6, dog6 = dog_ref.process_dog(v6, 8.0, 0.0, find_min=True, find_max=True)
    np.testing.assert_array_equal(d, dog6)
    assert len(exp6) > 0
    check_points(pts, exp6)
    # 7, 8: release the workspace; the first DoG again
    _lib.check(lib.spim_dog_release_workspace(0))
    check_largest_dog()
