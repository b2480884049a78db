"""GPU parity of the downsampling kernels against the restatement in
tests/downsample_ref.py: every voxel bit for bit (NaN for NaN, the sign of zero included),
then the detectors and the pipeline on downsampled views."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import dom_ref
import downsample_ref as dr
from oracle import dog_ref
from spim_registration_amd import _lib, dog, dom, downsample as ds, pipeline, synthetic
from test_downsample_cpu import BLOB_CENTRE, BLOB_SHAPE, blob_volume

pytestmark = pytest.mark.gpu

# k_ds_xy's tile of final outputs (csrc/downsample.hip: kDsTileX = 128 input columns, kDsTileY = 64
# input rows): (128 >> levels of x) x (64 >> levels of y)
TILE = {2: (64, 32), 4: (32, 16), 8: (16, 8)}


def same_bits(a, b):
    """equal float32 arrays, NaN for NaN and the sign of zero included"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape, (a.shape, b.shape)
    nan = np.isnan(b)
    np.testing.assert_array_equal(np.isnan(a), nan)
    np.testing.assert_array_equal(np.where(nan, np.float32(0), a).view(np.uint32),
                                  np.where(nan, np.float32(0), b).view(np.uint32))


def volume(shape, seed=None):
    rng = np.random.default_rng(sum(shape) if seed is None else seed)
    return ((rng.random(shape) - 0.25) * 4000).astype(np.float32)


def raw(img, factor_xyz):
    """spim_downsample with a factor per axis (x, y, z) on a host array"""
    lib = _lib.load()
    dims = (C.c_int64 * 3)(img.shape[2], img.shape[1], img.shape[0])
    f = (C.c_int32 * 3)(*factor_xyz)
    od = (C.c_int64 * 3)()
    _lib.check(lib.spim_downsample_dims(dims, f, od))
    out = np.empty((od[2], od[1], od[0]), np.float32)
    _lib.check(lib.spim_downsample(img.ctypes.data, dims, f, 0, out.ctypes.data))
    return out


def check(img, xy, z):
    """host array and device tensor against the restatement; the device input untouched"""
    want = dr.downsample(img, xy, z)
    got = ds.downsample(img, xy, z)
    assert isinstance(got, np.ndarray)
    same_bits(got, want)
    src = torch.from_numpy(np.array(img)).cuda()
    out = ds.downsample(src, xy, z)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32
    same_bits(out.cpu().numpy(), want)
    np.testing.assert_array_equal(src.cpu().numpy().view(np.uint32), np.asarray(img).view(np.uint32))
    return want


@pytest.mark.parametrize("axis", [0, 1, 2])       # numpy axis: z, y, x
@pytest.mark.parametrize("f", [2, 4, 8])
def test_edges_per_axis_and_factor(gpu, f, axis):
    """Every length from 2f (m = 2 at the last level: only the two edge formulas) to 6f + 1
    (all residues, the odd intermediate sizes) on one axis; the others 5-9 long, factor 1."""
    others = [(5, 7), (9, 6), (8, 5)][axis]
    for n in range(2 * f, 6 * f + 2):
        shape = list(others)
        shape.insert(axis, n)
        img = volume(tuple(shape), seed=100 * f + n)
        factor = [1, 1, 1]
        factor[2 - axis] = f
        want = img
        for _ in range(dr.levels(f)):
            want = dr.simple2x(want, axis)
        same_bits(raw(img, factor), want)


@pytest.mark.parametrize("shape,xy,z", [
    ((21, 37, 70), 2, 1),
    ((41, 132, 150), 4, 2),
    ((9, 150, 275), 8, 1),
    ((3, 2 * (TILE[2][1] + 1), 2 * (TILE[2][0] + 1)), 2, 1),       # outputs one past a tile: 33 x 65 of (66, 130)
    ((3, 4 * (TILE[4][1] + 1), 4 * (TILE[4][0] + 1)), 4, 1),       # 17 x 33 of (68, 132): rows read 16 bytes at a time
    ((2, 8 * (TILE[8][1] + 1) + 7, 8 * (TILE[8][0] + 1) + 4), 8, 1),   # 9 x 17 of (79, 140)
    ((81, 12, 16), 1, 8),                                          # the z kernel alone: 10 outputs, 4 per thread
    ((37, 9, 11), 2, 4),
    ((16, 16, 16), 8, 8),                                          # 2 x 2 x 2: edge formulas only
    ((5, 260, 8), 1, 1),
])
def test_tiles(gpu, shape, xy, z):
    want = check(volume(shape), xy, z)
    assert want.shape == dr.out_dims(shape, xy, z) == ds.out_dims(shape, xy, z)


def test_factor_one_returns_the_input_bits(gpu):
    img = volume((7, 9, 13))
    img[1, 2, 3], img[2, 3, 4], img[3, 3, 3] = np.nan, -0.0, np.float32(1e-42)
    for got in (ds.downsample(img), ds.downsample(torch.from_numpy(img).cuda()).cpu().numpy()):
        np.testing.assert_array_equal(got.view(np.uint32), img.view(np.uint32))


def test_row_loads_follow_the_pointer_alignment(gpu):
    """nx % 4 == 0 reads rows as float4 only from a 16-byte aligned image: the same view
    4 bytes into an allocation gives the same bits."""
    img = volume((6, 70, 136))
    want = dr.downsample(img, 4, 2)
    flat = torch.empty(img.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(img).cuda().reshape(-1)
    src = flat[1:].view(img.shape)
    assert src.is_contiguous() and src.data_ptr() % 16 == 4
    same_bits(ds.downsample(src, 4, 2).cpu().numpy(), want)
    same_bits(ds.downsample(torch.from_numpy(img).cuda(), 4, 2).cpu().numpy(), want)


def test_special_values(gpu):
    """NaN, +-inf, -0.0, float32 subnormals and 1e38 scattered in a random volume: a
    mismatch is a bug in the kernel's arithmetic or its denormal mode."""
    shape = (12, 44, 52)
    rng = np.random.default_rng(77)
    img = ((rng.random(shape) - 0.5) * 2).astype(np.float32)
    specials = np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 3e-39, -7e-40, 1.1754942e-38,
                           1e38, -1e38, 3e38, 3.4028235e38])
    idx = rng.choice(img.size, size=600, replace=False)
    img.reshape(-1)[idx] = specials[rng.integers(0, len(specials), size=600)]
    # runs of subnormals and of zeros of both signs, so that sums stay subnormal / signed zero
    img[2, 4:12, 8:20] = np.float32(1e-45) * rng.integers(1, 9, size=(8, 12)).astype(np.float32)
    img[6, 4:12, 8:16] = -0.0
    img[5, 20:28, 0:6] = np.float32(-2e-39)
    for xy, z in ((2, 1), (4, 2), (1, 4), (8, 1)):
        want = check(img, xy, z)
        assert np.isnan(want).any() and np.isinf(want).any()
    sub = dr.downsample(img, 2, 1)
    tiny = np.finfo(np.float32).tiny
    assert np.any((sub != 0) & (np.abs(sub) < tiny)) and np.any(np.signbit(sub) & (sub == 0))


def test_errors(gpu):
    with pytest.raises(ValueError):
        ds.downsample(volume((8, 8, 7)), 4, 1)              # 7 -> 3: the second level cannot be halved
    with pytest.raises(ValueError):
        ds.downsample(volume((8, 8, 8)), 3, 1)
    with pytest.raises(ValueError, match="3D"):
        ds.downsample(np.zeros((8, 8), np.float32), 2, 1)


@functools.lru_cache(maxsize=None)
def bead_stack():
    """The recipe of test_gpu_dom.bead_stack with a PSF wide enough to survive 2x in xy.
    Read-only: shared between tests."""
    shape = (40, 90, 97)
    rng = synthetic.rng_for(11)
    t = synthetic.truth_volume(shape, rng, bead_density=1.0 / 14 ** 3)
    k = synthetic.psf(0, 1, (17, 17, 13), sigma=(2.0, 2.0, 1.6))
    from oracle import mvdecon_ref as ref
    img = ref.convolve(t.astype(np.float32), k, "mirror")
    img = (rng.poisson(np.maximum(img * 2000 + 50, 0)) + rng.normal(0, 2, shape)).astype(np.float32)
    img.setflags(write=False)
    return img


def compare_points(pts, image, exp, exp_image, xy, z):
    """the detector's image bit for bit; the same ordered points and intensities, positions
    being correct_for_downsampling of the restatement's"""
    same_bits(np.asarray(image), exp_image)
    assert len(pts) == len(exp) > 0
    want = dr.correct_for_downsampling([e[:3] for e in exp], xy, z)
    got = np.array([p.location for p in pts], np.float64)
    print("max |position - expected|:", np.abs(got - want).max(), "max |intensity - expected|:",
          np.abs(np.float32([p.intensity for p in pts]) - np.float32([e[3] for e in exp])).max())
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(np.float32([p.intensity for p in pts]), np.float32([e[3] for e in exp]))


def test_dog_detection_on_a_downsampled_view(gpu):
    img = bead_stack()
    small = dr.downsample(img, 2, 1)
    exp, exp_dog = dog_ref.process_dog(small, localization=1)
    assert len(exp) == 36
    pts, d = dog.compute(img, localization=1, keep_intensity=True, return_dog=True, downsample_xy=2)
    assert d.shape == small.shape
    compare_points(pts, d, exp, exp_dog, 2, 1)
    src = torch.from_numpy(np.array(img)).cuda()
    pos, inten = dog.interest_points_array(src, localization=1, downsample_xy=2)
    np.testing.assert_array_equal(pos, np.array([p.location for p in pts]))
    np.testing.assert_array_equal(inten, np.float32([p.intensity for p in pts]))
    # full resolution: the half-size view's coordinates doubled in x and y only
    assert pos[:, 0].max() > small.shape[2] and pos[:, 2].max() < small.shape[0]


def test_dom_detection_on_a_downsampled_view(gpu):
    img = bead_stack()
    small = dr.downsample(img, 2, 1)
    exp, _, exp_dom = dom_ref.process_dom(small, localization=1)
    pts, d = dom.compute(img, localization=1, keep_intensity=True, return_dom=True, downsample_xy=2)
    compare_points(pts, d, exp, exp_dom, 2, 1)
    pos, inten = dom.interest_points_array(torch.from_numpy(np.array(img)).cuda(), localization=1, downsample_xy=2)
    np.testing.assert_array_equal(pos, np.array([p.location for p in pts]))
    np.testing.assert_array_equal(inten, np.float32([p.intensity for p in pts]))


def test_centred_blob(gpu):
    """A blob centred on voxel (4a, 4b, 2c) is found there: the correction is a pure scale."""
    img = blob_volume(BLOB_CENTRE, BLOB_SHAPE)
    for pts in (dog.compute(img, localization=1, downsample_xy=4, downsample_z=2),
                dog.compute(torch.from_numpy(img).cuda(), localization=1, downsample_xy=4, downsample_z=2)):
        assert len(pts) == 1
        assert np.abs(np.array(pts[0].location) - BLOB_CENTRE[::-1]).max() < 1e-3, pts[0].location


WORLD, PSF_SIZE = (48, 44, 40), (9, 9, 11)       # the timepoint of tests/test_gpu_pipeline.py


def test_pipeline_with_downsampling(gpu):
    views, models = synthetic.make_timepoint_torch(WORLD, WORLD, 4, timepoint=1, config_id=41,
                                                   bead_density=1.0 / 9 ** 3, device="cuda:0")
    kw = dict(psf_size=PSF_SIZE, iterations=1)
    res = pipeline.process_timepoint(views, models, (0, 0, 0), WORLD, downsample_xy=2, **kw)
    assert res.ms["detect"] >= res.ms["downsample"] > 0      # the pass alone, inside the detect stage
    direct = [dog.interest_points_array(v, sigma=1.8, threshold=0.008, localization=1, downsample_xy=2)
              for v in views]
    for pts, (pos, _) in zip(res.points, direct):
        assert len(pos) > 5
        np.testing.assert_array_equal(pts, pos)
    assert res.psi.shape == WORLD[::-1] and np.isfinite(res.psi.cpu().numpy()).all()
    # "Match Z Resolution": 2 from the voxel size
    same = pipeline.process_timepoint(views, models, (0, 0, 0), WORLD, downsample_xy="match_z_less",
                                      voxel_size=(0.4, 0.4, 1.0), **kw)
    for a, b in zip(same.points, res.points):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError):
        pipeline.process_timepoint(views, models, (0, 0, 0), WORLD, downsample_xy="match_z_less", **kw)
    for kind in ("brightest", "median", "weakest"):
        lim = pipeline.process_timepoint(views, models, (0, 0, 0), WORLD, downsample_xy=2, max_detections=5,
                                         max_detections_type=kind, **kw)
        for pts, (pos, inten) in zip(lim.points, direct):
            assert len(pts) == 5
            np.testing.assert_array_equal(pts, ds.limit_detections(pos, inten, 5, kind)[0])


def test_pipeline_defaults_are_unchanged(gpu):
    """Default arguments: the detectors' full-resolution calls, no downsampling entry, and
    the digest of a run that names every new parameter at its default."""
    views, models = synthetic.make_timepoint_torch(WORLD, WORLD, 4, timepoint=1, config_id=41,
                                                   bead_density=1.0 / 9 ** 3, device="cuda:0")
    kw = dict(psf_size=PSF_SIZE, iterations=2, digest=True)
    a = pipeline.process_timepoint(views, models, (0, 0, 0), WORLD, **kw)
    b = pipeline.process_timepoint(views, models, (0, 0, 0), WORLD, downsample_xy=1, downsample_z=1,
                                   voxel_size=None, max_detections=None, max_detections_type="brightest", **kw)
    assert "downsample" not in a.ms and "downsample" not in b.ms
    assert pipeline.result_digest(a) == pipeline.result_digest(b)
    for v, pts in zip(views, a.points):
        pos, _ = dog.interest_points_array(v, sigma=1.8, threshold=0.008, localization=1)
        np.testing.assert_array_equal(pts, pos)
