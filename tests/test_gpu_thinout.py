"""GPU parity of "Thin out detections" (csrc/thinout.hip) against the restatement in
tests/thinout_ref.py, bit for bit: the nearest-neighbour distances, the nearest indices, the kept
lists under both range rules, the histogram; then the pipeline's ``thin_out=``.

Bit for bit: equal uint64 views of the distances, of min, max and the bin centres; equal
integers.  tests/test_thinout_cpu.py holds the premises (what the cases contain)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import thinout_ref as tr
from spim_registration_amd import _lib, pipeline, synthetic, thinout

pytestmark = pytest.mark.gpu

ERR_ARG = -1
WORLD = (48, 44, 40)
PSF_SIZE = (9, 9, 11)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@functools.lru_cache(maxsize=None)
def case(seed, n, vox):
    return tr.make_case(seed, n, tr.VOXELS[vox])


@functools.lru_cache(maxsize=None)
def reference(seed, n, vox):
    """the restatement's (dist, nearest) of a case: computed once, shared, read-only"""
    return tr.nn_distances(case(seed, n, vox), tr.VOXELS[vox])


def check_thin_out(pts, voxel, want, lo=tr.MIN_D, hi=tr.MAX_D, **kw):
    """nn_distances and thin_out under both rules against (dist, nearest) of the restatement"""
    want_d, want_i = want
    d, i = thinout.nn_distances(pts, voxel, **kw)
    assert d.dtype == np.float64 and i.dtype == np.int32
    np.testing.assert_array_equal(bits(d), bits(want_d))
    np.testing.assert_array_equal(i, want_i)
    for keep_range in (False, True):
        out, kept, d, i = thinout.thin_out(pts, voxel, lo, hi, keep_range, return_all=True, **kw)
        want_k = np.nonzero(tr.keep_flags(want_d, lo, hi, keep_range))[0]
        assert kept.dtype == np.int32
        np.testing.assert_array_equal(kept, want_k)
        np.testing.assert_array_equal(bits(d), bits(want_d))
        np.testing.assert_array_equal(i, want_i)
        np.testing.assert_array_equal(bits(out), bits(np.asarray(pts, np.float64)[want_k]))


def test_tile_sizes_are_the_ones_the_cases_straddle(gpu):
    assert thinout.tile_sizes() == (tr.R_BLOCK, tr.C_TILE)


@pytest.mark.parametrize("vox", sorted(tr.VOXELS))
@pytest.mark.parametrize("seed,n", tr.SIZE_CASES)
def test_sizes(gpu, seed, n, vox):
    """2 and 3 points; one below / at / above the block of rows and the LDS tile; 2,500 points,
    where the automatic split takes more than one partition"""
    check_thin_out(case(seed, n, vox), tr.VOXELS[vox], reference(seed, n, vox))


@pytest.mark.parametrize("split", [1, 2, 7, 400])
def test_splits_give_identical_output(gpu, split):
    """t_split 1, 2, 7 and 400 (more partitions than the 333 points and the lattice's 216: some
    are empty), also where six neighbours tie across partitions"""
    seed, n = tr.SPLIT_CASE
    for vox in sorted(tr.VOXELS):
        check_thin_out(case(seed, n, vox), tr.VOXELS[vox], reference(seed, n, vox), t_split=split)
    lat = tr.lattice_case()
    check_thin_out(lat, (1.0, 1.0, 1.0), tr.nn_distances(lat), lo=0.5, hi=1.0, t_split=split)
    seed, n = tr.SIZE_CASES[-1]
    check_thin_out(case(seed, n, "aniso"), tr.VOXELS["aniso"], reference(seed, n, "aniso"), t_split=split)


def test_seams_and_duplicates(gpu):
    """the only near neighbour across the seam of the block of rows and of the LDS tile; exact
    duplicates: distance exactly 0 and the lower-indexed twin; the first and the last index of a
    tile are never their own neighbour"""
    pts, want = tr.seam_case()
    for split in (0, 1, 2):
        d, i = thinout.nn_distances(pts, t_split=split)
        for k, j in want.items():
            assert i[k] == j
        assert (i != np.arange(len(pts))).all()
        for k in (0, len(pts) - 1, 100, 300, 700):
            assert bits(d[k]) == bits(0.0)
        check_thin_out(pts, (1.0, 1.0, 1.0), tr.nn_distances(pts), lo=0.25, hi=50.0, t_split=split)


def test_thresholds_admit_equality(gpu):
    """max_distance exactly a point's distance: inside the range; the next double below: outside.
    min_distance exactly that distance: inside; the next double above: outside."""
    seed, n = 1, tr.R_BLOCK + 1
    pts, voxel = case(seed, n, "aniso"), tr.VOXELS["aniso"]
    want_d, _ = reference(seed, n, "aniso")
    k = int(np.argsort(want_d)[n // 2])
    d = float(want_d[k])
    assert 0.0 < d < 1e3
    below, above = float(np.nextafter(d, 0.0)), float(np.nextafter(d, np.inf))
    for lo, hi, inside in ((0.0, d, True), (0.0, below, False), (d, 1e6, True), (above, 1e6, False)):
        for keep_range in (False, True):
            _, kept, _, _ = thinout.thin_out(pts, voxel, lo, hi, keep_range, return_all=True)
            np.testing.assert_array_equal(kept, np.nonzero(tr.keep_flags(want_d, lo, hi, keep_range))[0])
            assert (k in kept) == (inside == keep_range)


def test_one_point_and_no_point(gpu):
    one = np.array([[3.0, 4.0, 5.0]])
    d, i = thinout.nn_distances(one)
    assert np.isposinf(d[0]) and list(i) == [-1]
    out, kept, d, i = thinout.thin_out(one, return_all=True)                 # remove-range keeps it
    assert list(kept) == [0] and np.isposinf(d[0]) and list(i) == [-1]
    np.testing.assert_array_equal(out, one)
    out, kept, _, _ = thinout.thin_out(one, keep_range=True, return_all=True)   # keep-range drops it
    assert len(kept) == 0 and out.shape == (0, 3)
    for keep_range in (False, True):
        out, kept, d, i = thinout.thin_out(np.zeros((0, 3)), keep_range=keep_range, return_all=True)
        assert out.shape == (0, 3) and len(kept) == len(d) == len(i) == 0
    d, i = thinout.nn_distances(np.zeros((0, 3)))
    assert len(d) == len(i) == 0
    # n == 0 through the C-ABI: the count is 0 and nothing else is touched
    p = _lib.ThinOutParams()
    _lib.load().spim_thinout_params_default(C.byref(p))
    count = C.c_int64(-7)
    vox = np.ones(3)
    _lib.check(_lib.load().spim_thin_out(None, 0, vox.ctypes.data_as(_lib._pd), C.byref(p), None, None, None, 0,
                                         C.byref(count)))
    assert count.value == 0


def check_histogram(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    assert got[1].dtype == np.int64
    np.testing.assert_array_equal(bits(got[0]), bits(want[0]))
    assert bits(got[2]) == bits(want[2]) and bits(got[3]) == bits(want[3])


def test_distance_histogram(gpu):
    """three views with different voxel sizes pooled; without and with a selection mask;
    subsampling=3 under the same draw; all distances equal; the maximum in the last bin"""
    views = [case(1, tr.C_TILE + 1, "iso"), case(1, tr.R_BLOCK - 1, "aniso"), case(2, 333, "iso")]
    voxels = [(1.0, 1.0, 1.0), (0.73, 0.73, 2.0), (0.5, 0.5, 1.3)]
    pooled = np.concatenate([tr.nn_distances(p, v)[0] for p, v in zip(views, voxels)])
    want = tr.histogram(pooled, bins=100)
    got = thinout.distance_histogram(views, voxels)
    check_histogram(got, want)
    assert got[1].sum() == len(pooled) and got[1][-1] >= 1
    sel = (np.arange(len(pooled)) % 5 != 1).astype(np.uint8)
    sel[pooled == pooled.max()] = 0                  # another maximum than the unmasked one
    check_histogram(thinout.histogram(pooled, sel, bins=37), tr.histogram(pooled, sel, bins=37))
    mask = np.random.default_rng(11).random(len(pooled)) < 1.0 / 3.0
    got = thinout.distance_histogram(views, voxels, bins=64, subsampling=3, seed=11)
    check_histogram(got, tr.histogram(pooled, mask, bins=64))
    assert got[1].sum() == mask.sum()
    check_histogram(thinout.histogram(np.full(300, 2.5), bins=10), tr.histogram(np.full(300, 2.5), bins=10))
    one_voxel = thinout.distance_histogram(views[:1], (1.0, 1.0, 1.0), bins=7)
    check_histogram(one_voxel, tr.histogram(reference(1, tr.C_TILE + 1, "iso")[0], bins=7))


def test_device_resident_input(gpu):
    """a CUDA tensor is read in place: the same result as from the host, and the returned points
    are the unscaled originals"""
    seed, n = tr.SIZE_CASES[-1]
    pts, voxel = case(seed, n, "aniso"), tr.VOXELS["aniso"]
    want_d, want_i = reference(seed, n, "aniso")
    dev = torch.from_numpy(pts).to("cuda:0")
    d, i = thinout.nn_distances(dev, voxel)
    np.testing.assert_array_equal(bits(d), bits(want_d))
    np.testing.assert_array_equal(i, want_i)
    host = thinout.thin_out(pts, voxel, tr.MIN_D, tr.MAX_D, return_all=True)
    out, kept, d, i = thinout.thin_out(dev, voxel, tr.MIN_D, tr.MAX_D, return_all=True)
    assert out.is_cuda and out.dtype == torch.float64
    np.testing.assert_array_equal(kept, host[1])
    np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(pts[kept]))
    np.testing.assert_array_equal(bits(host[0]), bits(pts[kept]))
    np.testing.assert_array_equal(bits(dev.cpu().numpy()), bits(pts))       # the input is untouched


def test_errors(gpu):
    lib = _lib.load()
    pts = case(1, 3, "iso").copy()

    def raises(fn, lead):
        with pytest.raises(_lib.SpimDeconError) as e:
            fn()
        assert e.value.status == ERR_ARG and _lib.last_error().startswith(lead), _lib.last_error()

    for bad in (np.nan, np.inf):
        q = pts.copy()
        q[1, 2] = bad
        raises(lambda: thinout.nn_distances(q), "thinout: non-finite coordinates")
        raises(lambda: thinout.thin_out(q), "thinout: non-finite coordinates")
    big = pts.copy()
    big[0, 0] = 1e300                      # finite as it stands, not after the scaling
    raises(lambda: thinout.nn_distances(big, (1e10, 1.0, 1.0)), "thinout: non-finite coordinates")
    raises(lambda: thinout.thin_out(pts, min_distance=5.0, max_distance=5.0), "thinout: min_distance")
    raises(lambda: thinout.thin_out(pts, min_distance=7.0, max_distance=5.0), "thinout: min_distance")
    raises(lambda: thinout.histogram(np.array([1.0])), "thinout: a histogram needs at least two points")
    raises(lambda: thinout.histogram(np.array([1.0, 2.0, 3.0]), np.zeros(3)), "thinout: a histogram of an empty")
    raises(lambda: thinout.histogram(np.array([1.0, np.inf])), "thinout: non-finite distances")
    raises(lambda: thinout.histogram(np.array([0.0, 1e12])), "thinout: a distance falls beyond the last bin")
    # capacity: three points are kept (remove-range, all farther apart than 1e-3), room for one
    p = _lib.ThinOutParams()
    lib.spim_thinout_params_default(C.byref(p))
    p.min_distance, p.max_distance = 0.0, 1e-3
    vox = np.ones(3)
    dist, nearest, kept = np.empty(3), np.empty(3, np.int32), np.full(3, -5, np.int32)
    count = C.c_int64(0)
    st = lib.spim_thin_out(C.c_void_p(pts.ctypes.data), 3, vox.ctypes.data_as(_lib._pd), C.byref(p),
                           C.c_void_p(dist.ctypes.data), C.c_void_p(nearest.ctypes.data),
                           C.c_void_p(kept.ctypes.data), 1, C.byref(count))
    assert st == ERR_ARG and count.value == 3
    assert _lib.last_error().startswith("thinout: 3 kept detections beyond the capacity 1")
    np.testing.assert_array_equal(bits(dist), bits(tr.nn_distances(pts)[0]))
    assert list(kept[1:]) == [-5, -5]


def test_pipeline_thin_out(gpu):
    """``thin_out=`` leaves ``points`` equal to thin_out applied to the points of the same call
    without it, is timed and logged; None is the keyword omitted"""
    views, models = synthetic.make_timepoint_torch(WORLD, WORLD, 4, timepoint=1, config_id=41,
                                                   bead_density=1.0 / 9 ** 3, device="cuda:0")
    kw = dict(psf_size=PSF_SIZE, iterations=1)
    plain = pipeline.process_timepoint(views, models, (0, 0, 0), WORLD, **kw)
    off = pipeline.process_timepoint(views, models, (0, 0, 0), WORLD, thin_out=None, **kw)
    assert pipeline.result_digest(off) == pipeline.result_digest(plain)
    assert "thin_out" not in plain.ms and "thin_out" not in off.ms
    for a, b in zip(plain.points, off.points):
        np.testing.assert_array_equal(bits(a), bits(b))
    voxel = (0.73, 0.73, 2.0)
    nn = np.sort(tr.nn_distances(plain.points[0], voxel)[0])
    d = float(nn[len(nn) // 4])                      # a quarter of view 0 goes
    lines = []
    res = pipeline.Pipeline(voxel_size=voxel, thin_out={"min_distance": 0, "max_distance": d}, **kw).process(
        views, models, (0, 0, 0), WORLD, log=lines.append)
    assert "thin_out" in res.ms and res.ms["thin_out"] <= res.ms["detect"]
    for v, (got, before) in enumerate(zip(res.points, plain.points)):
        want = thinout.thin_out(before, voxel, 0.0, d)
        np.testing.assert_array_equal(bits(got), bits(want))
        np.testing.assert_array_equal(bits(want), bits(tr.thin_out(before, voxel, 0.0, d)[0]))
        assert f"thin out: view {v}, detections: {len(before)} >>> {len(got)}" in lines
    assert 0 < len(res.points[0]) < len(plain.points[0])
    assert all((c < len(p)).all() for c, p in zip(res.corresponding, res.points))
