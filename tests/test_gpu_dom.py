"""GPU parity of the Difference-of-Mean detector against the restatement in
tests/dom_ref.py: the whole DOM image bit for bit, the exact ordered peak list, exact
float32 intensities."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import dom_ref as dr
from oracle import dog_ref
from spim_registration_amd import _lib, dog, dom, pipeline, synthetic

pytestmark = pytest.mark.gpu

NAN = float("nan")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dom.npz")


@functools.lru_cache(maxsize=None)
def bead_stack(shape=(40, 44, 48), cid=11):
    """The bead stack of the DoG tests (same recipe, restated): one partial 64-wide x
    strip, y and z no multiple of any tile.  Read-only: shared between tests."""
    rng = synthetic.rng_for(cid)
    t = synthetic.truth_volume(shape, rng, bead_density=1.0 / 10 ** 3)
    k = synthetic.psf(0, 1, (9, 9, 13), sigma=(1.0, 1.0, 1.6))
    from oracle import mvdecon_ref as ref
    img = ref.convolve(t.astype(np.float32), k, "mirror")
    img = (rng.poisson(np.maximum(img * 2000 + 50, 0)) + rng.normal(0, 2, shape)).astype(np.float32)
    img.setflags(write=False)
    return img


def same_bits(a, b):
    """equal float32 arrays, NaN for NaN and the sign of zero included"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    nan = np.isnan(b)
    np.testing.assert_array_equal(np.isnan(a), nan)
    np.testing.assert_array_equal(np.where(nan, np.float32(0), a).view(np.uint32),
                                  np.where(nan, np.float32(0), b).view(np.uint32))


def check(img, expect=None, device_tensor=False, **kw):
    """dom.compute (localization 0) against the restatement: image, ordered peaks, intensities.
    Returns the expected ordered peaks."""
    ref_kw = {k: v for k, v in kw.items() if k != "device"}
    exp_pts, exp_peaks, exp_dom = dr.process_dom(np.asarray(img), **ref_kw)
    src = torch.from_numpy(np.array(img)).cuda() if device_tensor else img
    pts, d = dom.compute(src, return_dom=True, keep_intensity=True, **kw)
    if device_tensor:
        assert isinstance(d, torch.Tensor) and d.is_cuda
        np.testing.assert_array_equal(src.cpu().numpy().view(np.uint32), np.asarray(img).view(np.uint32))  # input untouched
        d = d.cpu().numpy()
    same_bits(d, exp_dom)
    assert [tuple(int(c) for c in p.location) for p in pts] == [e[:3] for e in exp_pts]
    np.testing.assert_array_equal(np.float32([p.intensity for p in pts]), np.float32([e[3] for e in exp_pts]))
    if expect is not None:
        assert (sum(p[5] for p in exp_peaks), sum(p[4] for p in exp_peaks)) == expect
    return exp_peaks


TABLE = [   # (radius1, radius2, image sigma, threshold) -> (maxima, minima) of the bead stack
    ((2, 3, (0.5, 0.5, 0.5), 0.02), (12, 0)),
    ((2, 3, (0.5, 0.5, 0.5), 0.0025), (153, 786)),
    ((1, 2, (0.5, 0.5, 0.5), 0.02), (121, 12)),
    ((2, 3, (0.5, 0.5, 0.25), 0.02), (9, 39)),
    ((3, 2, (0.5, 0.5, 0.5), 0.02), (0, 12)),        # radius1 > radius2: the sign flipped exactly
]


@pytest.mark.parametrize("device_tensor", [False, True])
@pytest.mark.parametrize("setting,expect", TABLE)
def test_dom_matches_restatement(gpu, setting, expect, device_tensor):
    r1, r2, sigma, thr = setting
    peaks = check(bead_stack(), expect, device_tensor, radius1=r1, radius2=r2, image_sigma=sigma, threshold=thr,
                  find_min=True, find_max=True)
    assert len(peaks) > 0


def test_dom_sign_flip_is_exact(gpu):
    _, a = dom.compute(bead_stack(), radius1=2, radius2=3, return_dom=True)
    _, b = dom.compute(bead_stack(), radius1=3, radius2=2, return_dom=True)
    np.testing.assert_array_equal(a, -b)


@pytest.mark.parametrize("find_min,find_max,n", [(False, True, 153), (True, False, 786), (True, True, 939),
                                                 (False, False, 0)])
def test_dom_find_min_max(gpu, find_min, find_max, n):
    peaks = check(bead_stack(), threshold=0.0025, find_min=find_min, find_max=find_max)
    assert len(peaks) == n


@pytest.mark.parametrize("T", [1, 3, 8])
def test_dom_ij_threads_order(gpu, T):
    peaks = check(bead_stack(), threshold=0.0025, find_min=True, find_max=True, ij_threads=T)
    got = dom.simple_peaks(bead_stack(), threshold=0.0025, find_min=True, find_max=True, ij_threads=T)
    assert [g[:3] + g[4:] for g in got] == [p[:3] + p[4:] for p in peaks] and len(got) == 939
    np.testing.assert_array_equal(np.float32([g[3] for g in got]), np.float32([p[3] for p in peaks]))
    if T > 1:
        assert [p[:3] for p in peaks] != sorted((p[:3] for p in peaks), key=lambda q: (q[2], q[1], q[0]))


def test_dom_given_intensity_range(gpu):
    peaks = check(bead_stack(), threshold=0.004, min_intensity=0.0, max_intensity=4000.0, find_min=True)
    assert len(peaks) > 0
    # an unusable range (equal) falls back to the image's own
    a = check(bead_stack(), min_intensity=5.0, max_intensity=5.0)
    assert len(a) == 12


@pytest.mark.parametrize("factor,rounds", [(30, False), (2000, True)])
def test_dom_long_to_float_rounding_decides_bits(gpu, factor, rounds):
    """The stack scaled up: x 30 (peaks near 60 000; its largest box sum stays below 2^24 on
    this stack) and x 2000, where box sums exceed 2^24 and (float) long rounds."""
    img = (bead_stack() * np.float32(factor)).astype(np.float32)
    sums = dr.box_sums(dr.integral_image(img), (7, 7, 7), (3, 3, 3))
    if rounds:
        assert sums.max() > 2 ** 24 and np.any(sums.astype(np.float32).astype(np.int64) != sums)
    for dev in (False, True):
        assert len(check(img, device_tensor=dev, find_min=True)) > 0


def test_dom_negative_fractional_nan_and_saturating_voxels(gpu):
    rng = np.random.default_rng(7)
    img = ((rng.random((20, 22, 70)) - 0.4) * 3000).astype(np.float32)
    img[3, 4, 5] = 3e9
    img[10, 11, 40] = -3e9
    img[15, 3, 66] = np.inf
    # the image's own range is infinite: d = inf, every supported voxel +-0 or NaN
    check(img, find_min=True)
    peaks = check(img, min_intensity=-1200.0, max_intensity=1800.0, find_min=True, threshold=0.01)
    assert len(peaks) > 0
    img[7, 8, 9] = NAN
    peaks = check(img, min_intensity=-1200.0, max_intensity=1800.0, find_min=True, threshold=0.01)   # NaN -> 0
    assert len(peaks) > 0
    # FusionHelper.minMax keeps the NaN: the whole support is NaN, no peak
    pts, d = dom.compute(img, return_dom=True)
    assert pts == [] and np.isnan(d[3:-3, 3:-3, 3:-3]).all() and not d[:3].any()
    check(img)


def test_dom_largest_box(gpu):
    """Radii 15, 16: diameters 31 / 33, an 8 x 12 x 16 interior."""
    assert dom.box_diameters(15, 16) == ((31, 31, 31), (33, 33, 33))
    img = bead_stack()
    for dev in (False, True):
        check(img, device_tensor=dev, radius1=15, radius2=16, threshold=1e-4, find_min=True)
    _, d = dom.compute(img, radius1=15, radius2=16, return_dom=True)
    assert np.count_nonzero(d) > 0 and not d[:16].any() and np.all(d[16:24, 16:28, 16:32] != 0)
    with pytest.raises(_lib.SpimDeconError, match="33"):      # beyond the kernel's limit: an error, no image
        dom.compute(img, radius1=16, radius2=17)


@pytest.mark.parametrize("shape,kw", [
    ((7, 7, 7), {}),                                   # exactly one supported voxel
    ((7, 9, 6), {}),                                   # nx = 2 hm: all zero
    ((6, 9, 11), {}),                                  # nz = 2 hm
    ((9, 8, 65), {}),                                  # strip edges
    ((9, 8, 129), {}),
    ((8, 30, 21), {}),                                 # nz = 8 with diameter 7
    ((13, 7, 7), {"image_sigma": (0.5, 0.5, 0.25)}),   # one voxel of an anisotropic box
    ((3, 3, 3), {}),
    ((1, 1, 1), {}),
])
def test_dom_edge_shapes(gpu, shape, kw):
    rng = np.random.default_rng(sum(shape))
    img = (rng.random(shape) * 4000).astype(np.float32)
    for dev in (False, True):
        check(img, device_tensor=dev, threshold=0.001, find_min=True, **kw)
    _, d = dom.compute(img, return_dom=True, **kw)
    hm = [s // 2 for s in dr.box_diameters(2, 3, kw.get("image_sigma", (0.5, 0.5, 0.5)))[1]]
    fits = all(n > 2 * h for n, h in zip(shape[::-1], hm))
    assert (np.count_nonzero(d) > 0) == fits


@pytest.mark.parametrize("name", list(dr.Z_CHUNK_CASES))
def test_dom_across_z_chunks(gpu, name):
    """More output planes than one block walks (max(64, 8 hm_z)): the running z sums start
    afresh at the second chunk -- ragged and full last chunks, the 128-plane chunk of the
    largest box (16 columns per thread), and a 96-plane chunk with hm_z != hm_x."""
    shape, kw, chunks = dr.Z_CHUNK_CASES[name]
    img = dr.z_chunk_volume(name)
    for dev in (False, True):
        peaks = check(img, device_tensor=dev, threshold=0.001, find_min=True, **kw)
    hm_z = (shape[0] - sum(chunks)) // 2
    assert {p[2] for p in peaks} >= {hm_z + chunks[0] - 1, hm_z + chunks[0]} or name == "largest_box"
    assert len(peaks) > 0


def test_dom_integer_plateaus_across_z_chunks(gpu):
    """Sparse small integers: box sums tie, whole regions share one DOM value; >= and <= and
    the MAX-first rule decide, on both sides of the chunk seam."""
    img = dr.sparse_integer_volume()
    for dev in (False, True):
        peaks = check(img, device_tensor=dev, threshold=0.0, find_min=True, find_max=True)
    assert len(peaks) > 1000


def test_dom_constant_image(gpu):
    """diff = 0: NaN where the boxes fit, the zero frame around it, no peaks."""
    for value in (0.0, 7.0, -3.5):
        img = np.full((12, 13, 14), value, np.float32)
        assert check(img, find_min=True) == []
        pts, d = dom.compute(img, return_dom=True)
        assert pts == [] and np.isnan(d[3:-3, 3:-3, 3:-3]).all() and np.count_nonzero(np.nan_to_num(d)) == 0


def test_dom_quadratic_localization_takes_candidates_at_the_threshold(gpu):
    """ProcessDOM.java:104: no threshold / 10, unlike ProcessDOG."""
    img = bead_stack(cid=13)
    thr = 0.02
    _, _, d = dr.process_dom(img, threshold=thr, find_min=True)
    at_thr = dog_ref.find_peaks(d, float(np.float32(thr)))
    at_tenth = dog_ref.find_peaks(d, float(np.float32(thr) / np.float32(10)))
    assert len(at_tenth) > len(at_thr) > 0      # the two candidate lists differ on this stack
    exp, _, _ = dr.process_dom(img, threshold=thr, localization=1, find_min=True)
    got = dom.simple_peaks(img, threshold=thr, localization=1, find_min=True)
    assert [g[:3] for g in got] == [p[:3] for p in at_thr]
    pts, dgot = dom.compute(img, threshold=thr, localization=1, find_min=True, return_dom=True, keep_intensity=True)
    same_bits(dgot, d)
    assert len(pts) == len(exp) > 5
    gotp = np.array([p.location for p in pts])
    want = np.array([e[:3] for e in exp])
    # the comparison of tests/test_gpu_dog.py::test_dog_quadratic_localization
    np.testing.assert_allclose(gotp, want, rtol=0, atol=1e-5)
    np.testing.assert_allclose([p.intensity for p in pts], [e[3] for e in exp], rtol=1e-6, atol=1e-9)
    assert np.any(np.abs(gotp - np.round(gotp)) > 1e-3)      # genuinely sub-pixel
    pos, inten = dom.interest_points_array(torch.from_numpy(np.array(img)).cuda(), threshold=thr, localization=1,
                                           find_min=True)
    np.testing.assert_array_equal(pos, gotp)
    np.testing.assert_array_equal(inten, np.float32([p.intensity for p in pts]))


def test_dom_localization_2_is_an_error(gpu):
    with pytest.raises(_lib.SpimDeconError, match="localization must be 0"):
        dom.compute(bead_stack(), localization=2)


def test_dom_and_dog_share_the_workspace(gpu):
    a, b = bead_stack(), bead_stack(shape=(24, 26, 30), cid=12)
    lib = _lib.load()

    def run_dom(img):
        pts, d = dom.compute(img, threshold=0.0025, find_min=True, return_dom=True, keep_intensity=True)
        return [(p.location, p.intensity) for p in pts], d

    def run_dog(img):
        pts, d = dog.compute(img, localization=1, return_dog=True, keep_intensity=True)
        return [(p.location, p.intensity) for p in pts], d
    dog_b, dom_a, dog_a = run_dog(b), run_dom(a), run_dog(a)
    dom_b = run_dom(b)
    assert len(dom_a[0]) == 939 and len(dog_a[0]) > 5
    assert lib.spim_dog_release_workspace(0) == 0
    for first, again in ((dom_a, run_dom(a)), (dog_b, run_dog(b)), (dom_b, run_dom(b)), (dog_a, run_dog(a))):
        assert first[0] == again[0]
        np.testing.assert_array_equal(first[1], again[1])
    _, peaks, d = dr.process_dom(a, threshold=0.0025, find_min=True)
    same_bits(dom_a[1], d)


def test_dom_golden(gpu):
    g = np.load(GOLDEN)
    got, d = dom.simple_peaks(g["img"], find_min=True, return_dom=True)
    same_bits(d, g["dom"])
    assert [(p[0], p[1], p[2], int(p[4]), int(p[5])) for p in got] == [tuple(r) for r in g["peaks"].tolist()]
    np.testing.assert_array_equal(np.float32([p[3] for p in got]), g["intensity"])
    assert len(got) > 5


def test_dom_capacity_rule(gpu):
    img = np.ascontiguousarray(bead_stack())
    lib = _lib.load()
    p = _lib.DomParams()
    lib.spim_dom_params_default(C.byref(p))
    p.threshold, p.find_min = 0.0025, 1
    dims = (C.c_int64 * 3)(48, 44, 40)
    n = C.c_int64(0)
    pk = (_lib.Peak * 10)()
    assert lib.spim_dom_compute(_lib.fptr(img), dims, C.byref(p), None, pk, 10, C.byref(n)) == 0
    assert n.value == 939      # the total; only 10 were written
    full = dom.simple_peaks(img, threshold=0.0025, find_min=True)
    assert [(q.x, q.y, q.z) for q in pk] == [f[:3] for f in full[:10]]
    assert lib.spim_dom_compute(_lib.fptr(img), dims, C.byref(p), None, None, 0, C.byref(n)) == 0 and n.value == 939


def test_pipeline_with_the_dom_detector(gpu):
    """The small instance of tests/test_gpu_pipeline.py, scaled to camera counts (DOM sums
    (int) voxels: the instance's [0, 0.5] range would be all zero)."""
    world, psf_size = (48, 44, 40), (9, 9, 11)
    views, models = synthetic.make_timepoint_torch(world, world, 4, timepoint=1, config_id=41,
                                                   bead_density=1.0 / 9 ** 3, device="cuda:0")
    views = [v * 8000.0 for v in views]
    res = pipeline.process_timepoint(views, models, (0, 0, 0), world, psf_size=psf_size, iterations=2,
                                     detector="dom", radius1=2, radius2=3, threshold=0.02)
    for v, pts in zip(views, res.points):
        pos, _ = dom.interest_points_array(v, radius1=2, radius2=3, threshold=0.02, localization=1)
        np.testing.assert_array_equal(pts, pos)
        exp, _, _ = dr.process_dom(v.cpu().numpy(), threshold=0.02, localization=1)
        assert len(exp) > 3
        np.testing.assert_allclose(pts, np.array([e[:3] for e in exp]), rtol=0, atol=1e-5)
    psi = res.psi.cpu().numpy()
    assert psi.shape == world[::-1] and np.isfinite(psi).all() and (psi > 0).mean() > 0.5
