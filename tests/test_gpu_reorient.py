"""GPU parity of the reorienting bounding box (csrc/reorient.hip) against the restatement in
tests/reorient_ref.py, bit for bit: equal uint64 views of every float64 and equal integers.
(The restatement calls the same libm for sqrt, acos, sin and cos as the library's host side;
parity with a JVM's Math is not pinned.  Where a box is NaN only its NaN-ness is compared.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import reorient_ref as rr
from spim_registration_amd import _lib, boundingbox as bb, pipeline, synthetic

pytestmark = pytest.mark.gpu

T = 256   # the kernel's tile (test_tile_is_the_one_the_cases_straddle)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def cloud(n, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).normal(0.0, 40.0, (n, 3)))


def check_pair(pts, want=None):
    want = rr.farthest_pair(pts) if want is None else want
    got = bb.farthest_pair(pts)
    assert got[:2] == want[:2]
    assert bits(got[2]) == bits(want[2])
    return got


def test_tile_is_the_one_the_cases_straddle(gpu):
    assert bb.reorient_tile() == T


# ---------------------------------------------------------------- farthest pair
@pytest.mark.parametrize("n", [2, 3, T - 1, T, T + 1, 2 * T + 1])
def test_farthest_pair_sizes(gpu, n):
    """two and three points, one below / at / above the tile, two tiles and one point (three row
    tiles, where the automatic split gives more partitions than the last rows have tiles)"""
    check_pair(cloud(n, 100 + n))


@pytest.mark.parametrize("n,i,j", [(600, 300, 400), (600, 10, 500), (600, 520, 590), (600, 5, 599),
                                   (T + 1, 0, T), (T + 1, T - 1, T), (2 * T, T - 1, T)])
def test_farthest_pair_winner_position(gpu, n, i, j):
    """the winner inside a diagonal tile, in an off-diagonal tile, inside the last partial tile,
    from the first tile into the last point; across the tile seam"""
    pts = cloud(n, 7 * n + i)
    pts[i] = (-500.0, 3.0, 1.0)
    pts[j] = (500.0, -2.0, 4.0)
    assert check_pair(pts)[:2] == (i, j)
    pts[[i, j]] = pts[[j, i]]                 # the row point has the larger x: swapped
    assert check_pair(pts)[:2] == (j, i)


def test_farthest_pair_ties_across_blocks(gpu):
    """every point of a 9 x 9 x 9 integer lattice, shuffled (729 points: three row tiles): the four
    body diagonals tie exactly, and their end points fall into different blocks; the first pair
    in scan order wins.  Then with the winner's pair moved to the end: another diagonal wins."""
    rng = np.random.default_rng(42)
    lat = np.array([[x, y, z] for x in range(9) for y in range(9) for z in range(9)], np.float64)
    pts = np.ascontiguousarray(rng.permutation(lat))
    corner = np.flatnonzero(np.all((pts == 0) | (pts == 8), axis=1))
    assert len(corner) == 8 and len({c // T for c in corner}) > 1      # in more than one tile
    want = rr.farthest_pair(pts)
    assert want == rr.farthest_pair_literal(pts) and want[2] == 192.0
    first = check_pair(pts, want)
    assert min(first[:2]) == corner[0]                                  # the first corner's diagonal
    other = np.ascontiguousarray(np.concatenate([np.delete(pts, list(first[:2]), axis=0), pts[list(first[:2])]]))
    second = check_pair(other)
    assert second[2] == 192.0 and max(second[:2]) < len(pts) - 2


def test_farthest_pair_start_pair_and_x_order(gpu):
    """the cases of tests/test_reorient_cpu.py::test_farthest_pair_known_answers, and the start
    pair (0, 1) with points[0].x > points[1].x winning over a later tie in another tile"""
    for pts, want in (([[0, 0, 0], [3, 4, 0]], (0, 1, 25.0)), ([[3, 4, 0], [0, 0, 0]], (0, 1, 25.0)),
                      ([[9, 0, 0], [-9, 0, 0], [0, 1, 0], [1, 0, 1]], (0, 1, 324.0)),
                      ([[9, 0, 0], [-9, 0, 0], [0, 9, 0], [0, -9, 0]], (0, 1, 324.0)),
                      ([[0, 0, 0], [1, 0, 0], [5, 0, 0], [-5, 1, 0]], (3, 2, 101.0)),
                      ([[0, 0, 0], [1, 0, 0], [2, 7, 0], [2, -7, 0]], (2, 3, 196.0)),
                      ([[0, 0, 0], [1, 0, 0], [0, 6, 0], [0, -6, 0], [-6, 0, 0], [6, 0, 0]], (2, 3, 144.0))):
        assert check_pair(np.array(pts, np.float64)) == want
    pts = cloud(2 * T + 40, 3) * 0.01
    pts[0], pts[1] = (70.0, 0.0, 0.0), (-70.0, 0.0, 0.0)
    pts[T + 5], pts[2 * T + 7] = (0.0, 70.0, 0.0), (0.0, -70.0, 0.0)
    assert check_pair(pts) == (0, 1, 19600.0)


def test_device_input_equals_host_input(gpu):
    pts = cloud(2 * T + 1, 77)
    dp = torch.from_numpy(pts.copy()).cuda()
    want = rr.farthest_pair(pts)
    got = bb.farthest_pair(dp)
    assert got[:2] == want[:2] and bits(got[2]) == bits(want[2])
    mats = [rr.rotation(rr.normalize((0.2, 0.9, -0.4)), rr.X_AXIS), rr.identity()]
    np.testing.assert_array_equal(bits(bb.axis_boxes(dp, mats)), bits(rr.axis_boxes(pts, mats)))
    np.testing.assert_array_equal(bits(bb.points_min_max(dp)), bits(bb.points_min_max(pts)))
    assert np.array_equal(dp.cpu().numpy(), pts)                        # the input is untouched


# ---------------------------------------------------------------- axis boxes
def search_matrices(sv, step):
    """the 27 candidates of one scale step, in zi, yi, xi order"""
    return [rr.rotation(rr.normalize((sv[0] + xi * step, sv[1] + yi * step, sv[2] + zi * step)), rr.X_AXIS)
            for zi in (-1, 0, 1) for yi in (-1, 0, 1) for xi in (-1, 0, 1)]


@functools.lru_cache(maxsize=None)
def mats27():
    return np.array(search_matrices(rr.normalize((0.5, -0.3, 0.8)), 0.4))


@pytest.mark.parametrize("m", [1, 27])
@pytest.mark.parametrize("n", [1, T - 1, T + 1, 4 * T + 3])
def test_axis_boxes_sizes(gpu, n, m):
    """one point, around the block, and more than one block of points per matrix"""
    pts = cloud(n, 200 + n)
    mats = mats27()[:m] if m > 1 else mats27()[13:14]
    got = bb.axis_boxes(pts, mats)
    assert got.shape == (m, 6)
    np.testing.assert_array_equal(bits(got), bits(rr.axis_boxes(pts, mats)))


def test_axis_boxes_nan_matrix_stays_alone(gpu):
    pts = cloud(T + 1, 9)
    mats = mats27().copy()
    mats[5] = np.nan
    mats[20, 1, 2] = np.nan                    # one entry: the y row only
    got, want = bb.axis_boxes(pts, mats), rr.axis_boxes(pts, mats)
    assert np.isnan(got[5]).all() and np.isnan(want[5]).all()
    assert np.isnan(got[20, [1, 4]]).all() and not np.isnan(got[20, [0, 2, 3, 5]]).any()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got[ok]), bits(want[ok]))
    assert ok.sum() == 27 * 6 - 6 - 2


def test_axis_boxes_negative_zero(gpu):
    """-0.0 coordinates: Transform3D.transform under the identity ends in "+ 0.0", which makes
    them +0.0; the plain min / max keeps them, and -0.0 < +0.0 for Math.min, not for Math.max"""
    pts = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, -0.0], [5.0, 7.0, -0.0]])
    got = bb.axis_boxes(pts, [rr.identity()])
    want = rr.axis_boxes(pts, [rr.identity()])
    np.testing.assert_array_equal(bits(got), bits(want))
    assert not np.signbit(got[0, :3]).any()
    raw = bb.points_min_max(pts)
    lo, hi = rr.size_simple(pts)
    np.testing.assert_array_equal(bits(raw), bits(lo + hi))
    assert np.signbit(raw).tolist() == [True, True, True, False, False, True]
    neg = np.array([[-0.0, -1.0, -1.0], [-0.0, -2.0, -3.0]])            # x = -0 * 1 + ... + 0.0
    np.testing.assert_array_equal(bits(bb.axis_boxes(neg, [rr.identity()])), bits(rr.axis_boxes(neg, [rr.identity()])))


# ---------------------------------------------------------------- end to end
def check_whole(lists, models, corr, percent, reorientate, device_lists=None, **kw):
    want = rr.reorient_bounding_box(lists, models, corr, percent, reorientate)
    transform, new_models, bb_min, bb_dims, det = bb.reorient_bounding_box(
        lists if device_lists is None else device_lists, models, corresponding=corr, percent=percent, reorientate=reorientate, return_details=True, **kw)
    np.testing.assert_array_equal(bits(transform), bits(want["transform"]))
    np.testing.assert_array_equal(bits(det["min_f"]), bits(want["min_f"]))
    np.testing.assert_array_equal(bits(det["max_f"]), bits(want["max_f"]))
    assert (bb_min, det["bb_max"], bb_dims) == (want["bb_min"], want["bb_max"], want["bb_dims"])
    assert len(new_models) == len(models)
    for g, w in zip(new_models, want["new_models"]):
        np.testing.assert_array_equal(bits(g), bits(w))
    assert det["n_points"] == len(want["points"])
    if reorientate:
        assert det["far_pair"] == want["far_pair"] and bits(det["far_d2"]) == bits(want["far_d2"])
        assert bits(det["start_volume"]) == bits(want["start_volume"])
        assert bits(det["min_volume"]) == bits(want["min_volume"])
        np.testing.assert_array_equal(bits(det["axis"]), bits(want["axis"]))
    else:
        assert det["far_pair"] == (-1, -1)
    return want, det


@pytest.mark.parametrize("reorientate", [True, False])
@pytest.mark.parametrize("use_corr", [False, True])
def test_whole_call_on_the_cuboid(gpu, use_corr, reorientate):
    """the cuboid of tests/test_reorient_cpu.py over 3 views with non-trivial models: all
    detections and the corresponding subsets, reorientated and plain"""
    lists, models, corr = rr.cuboid_views()
    want, det = check_whole(lists, models, corr if use_corr else None, 10.0, reorientate)
    if reorientate:
        assert det["min_volume"] < 0.06 * rr.volume_of(rr.box_of(want["points"]))
    check_whole(lists, models, corr if use_corr else None, 0.0, reorientate)


def test_whole_call_partitions_and_device_lists(gpu):
    lists, models, corr = rr.cuboid_views()
    for split in (1, 2, 5):    # forced partitions of the column tiles (400 points: 2 tiles)
        check_whole(lists, models, None, 10.0, True, far_split=split)
    dl = [torch.from_numpy(p.copy()).cuda() for p in lists]
    check_whole(lists, models, corr, 25.0, True, device_lists=dl)
    big = [cloud(3 * T + 17, 5), cloud(T, 6)]                           # four row tiles
    ident = [rr.identity(), rr.identity()]
    for split in (0, 3):
        check_whole(big, ident, None, 10.0, True, far_split=split)


# ---------------------------------------------------------------- errors
def test_errors_name_the_call(gpu, lib):
    one = np.array([[1.0, 2.0, 3.0]])
    ident = [rr.identity()]
    for call, who in ((lambda: bb.farthest_pair(one), "farthest_pair"),
                      (lambda: bb.reorient_bounding_box([one], ident), "reorient"),
                      (lambda: bb.reorient_bounding_box([cloud(5, 1)], ident, corresponding=[[3]]), "reorient"),
                      (lambda: bb.axis_boxes(np.zeros((0, 3)), ident), "axis_boxes")):
        with pytest.raises(_lib.SpimDeconError) as e:
            call()
        assert e.value.status == -1 and who + ":" in str(e.value) and "point" in str(e.value)
    transform, _, bb_min, bb_dims = bb.reorient_bounding_box([one], ident, reorientate=False)   # one point: plain
    assert bb_min == (1, 2, 3) and bb_dims == (1, 1, 1)
    for bad in (np.nan, np.inf, 1e300):       # (1e300 is not finite as a float: the matchers' rule)
        x = cloud(300, 2)
        x[280, 1] = bad
        for call, who in ((lambda: bb.farthest_pair(x), "farthest_pair"), (lambda: bb.axis_boxes(x, ident), "axis_boxes"),
                          (lambda: bb.points_min_max(x), "points_min_max"),
                          (lambda: bb.reorient_bounding_box([cloud(9, 1), x], ident * 2), "reorient")):
            with pytest.raises(_lib.SpimDeconError) as e:
                call()
            assert e.value.status == -1 and who + ": non-finite" in str(e.value)
    with pytest.raises(_lib.SpimDeconError) as e:      # finite lists, not finite under the model
        bb.reorient_bounding_box([cloud(9, 1)], [rr.identity() * 1e308])
    assert e.value.status == -1 and "reorient: non-finite" in str(e.value)
    with pytest.raises(_lib.SpimDeconError) as e:
        bb.reorient_bounding_box([cloud(9, 1)], ident, corresponding=[[0, 9]])
    assert e.value.status == -1 and "reorient: corresponding index out of range" in str(e.value)
    # a null list with a positive count
    i, j, d = C.c_int32(), C.c_int32(), C.c_double()
    out = np.zeros(6)
    assert lib.spim_farthest_pair(None, 5, 0, C.byref(i), C.byref(j), C.byref(d)) == -1
    assert "farthest_pair: null point list" in _lib.last_error()
    assert lib.spim_points_min_max(None, 5, 0, out.ctypes.data_as(_lib._pd)) == -1
    assert "points_min_max: null point list" in _lib.last_error()
    p, r = _lib.ReorientParams(), _lib.ReorientResult()
    lib.spim_reorient_params_default(C.byref(p))
    p.use_corresponding = 0
    lists, counts = (C.c_void_p * 1)(None), (C.c_int64 * 1)(4)
    m = np.ascontiguousarray(rr.identity().reshape(12))
    assert lib.spim_reorient_bounding_box(1, lists, counts, None, None, m.ctypes.data_as(_lib._pd), C.byref(p),
                                          C.byref(r)) == -1
    assert "reorient: null point list" in _lib.last_error()
    check_pair(cloud(300, 2))                 # the next call is not affected
    bb.release_reorient_workspace(0)
    check_pair(cloud(300, 2))                 # (the workspace comes back)


# ---------------------------------------------------------------- pipeline
WORLD = (48, 44, 40)   # the timepoint of tests/test_gpu_pipeline.py and of test_gpu_autobbox.py's pipeline test


def test_process_timepoint_reorient(gpu):
    """bb_min="reorient": the box, the transform and the models are what reorient_bounding_box
    (and the restatement) give for the result's points, corresponding detections and the input
    models; psi is finite and of that box's shape; an explicit box leaves reorientation None"""
    views, models = synthetic.make_timepoint_torch(WORLD, WORLD, 4, timepoint=1, config_id=41,
                                                   bead_density=1.0 / 9 ** 3, device="cuda:0")
    kw = dict(psf_size=(9, 9, 11), iterations=1)
    lines = []
    res = pipeline.process_timepoint(views, models, "reorient", log=lines.append, **kw)
    assert sum(len(c) for c in res.corresponding) >= 2
    transform, new_models, bb_min, bb_dims = bb.reorient_bounding_box(res.points, models,
                                                                      corresponding=res.corresponding)
    want = rr.reorient_bounding_box(res.points, models, res.corresponding, 10.0, True)
    assert res.bounding_box == (bb_min, bb_dims) == (want["bb_min"], want["bb_dims"])
    np.testing.assert_array_equal(bits(res.reorientation), bits(transform))
    np.testing.assert_array_equal(bits(transform), bits(want["transform"]))
    for g, w in zip(res.models, new_models):
        np.testing.assert_array_equal(bits(g), bits(w))
    assert "reorient_bounding_box" in res.ms and any("reorienting bounding box" in ln for ln in lines)
    assert tuple(res.psi.shape) == bb_dims[::-1] and bool(torch.isfinite(res.psi).all())
    allp = pipeline.process_timepoint(views, models, "reorient", reorient={"corresponding": False, "percent": 0.0},
                                      **kw)
    a_t, _, a_min, a_dims = bb.reorient_bounding_box(res.points, models, percent=0.0)
    assert allp.bounding_box == (a_min, a_dims)
    np.testing.assert_array_equal(bits(allp.reorientation), bits(a_t))
    explicit = pipeline.process_timepoint(views, models, (0, 0, 0), WORLD, **kw)
    assert explicit.reorientation is None and "reorient_bounding_box" not in explicit.ms
    for g, w in zip(explicit.models, models):
        np.testing.assert_array_equal(g, np.asarray(w, np.float64).reshape(3, 4))
    with pytest.raises(ValueError):
        pipeline.process_timepoint(views, models, "reorient", WORLD, **kw)
    with pytest.raises(ValueError):
        pipeline.process_timepoint(views, models, (0, 0, 0), WORLD, reorient={}, **kw)
    with pytest.raises(ValueError):
        pipeline.process_timepoint(views, models, "reorient", auto_bb={}, **kw)
