"""CPU: the restatement of the reorienting bounding box (tests/reorient_ref.py) against
independent answers -- a brute force over the full distance matrix, hand-made pairs, properties
of the rotation, a cuboid whose own box is known, hand-rounded paddings -- and the parts of the
feature that need no GPU (the exported defaults, the Python composition of the models)."""
import ctypes as C
import math

import numpy as np
import pytest

import reorient_ref as rr
from spim_registration_amd import _lib, boundingbox as bb


def brute_force_pair(pts):
    """np.argmax over the full matrix (row-major: the first pair in scan order among the
    largest), then the reference's order of the pair"""
    pts = np.asarray(pts, np.float64)
    d = pts[:, None, :] - pts[None, :, :]
    d = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    d[np.tril_indices(len(pts))] = -1.0
    i, j = np.unravel_index(np.argmax(d), d.shape)
    if (i, j) != (0, 1) and not pts[i, 0] <= pts[j, 0]:
        i, j = j, i
    return int(i), int(j), float(d.max())


@pytest.mark.parametrize("n,seed,lattice", [(2, 1, False), (3, 2, False), (57, 3, False), (200, 4, False),
                                            (64, 5, True), (125, 6, True)])
def test_farthest_pair_equals_brute_force(n, seed, lattice):
    rng = np.random.default_rng(seed)
    if lattice:      # every point of a cubic lattice, shuffled: its four body diagonals tie
        k = round(n ** (1.0 / 3.0))
        pts = rng.permutation(np.array([[x, y, z] for x in range(k) for y in range(k) for z in range(k)], np.float64))
    else:
        pts = rng.normal(0.0, 50.0, (n, 3))
    want = brute_force_pair(pts)
    assert rr.farthest_pair_literal(pts) == want
    assert rr.farthest_pair(pts) == want
    if lattice:      # many pairs at the largest distance: the rule has something to decide
        d = np.linalg.norm(pts[:, None] - pts[None], axis=2) ** 2
        assert np.count_nonzero(np.triu(np.isclose(d, want[2]), 1)) == 4


def test_farthest_pair_known_answers():
    assert rr.farthest_pair([[0, 0, 0], [3, 4, 0]]) == (0, 1, 25.0)
    assert rr.farthest_pair([[3, 4, 0], [0, 0, 0]]) == (0, 1, 25.0)          # two points: never reordered
    # (0, 1) wins with points[0].x > points[1].x: stays (0, 1)
    pts = [[9, 0, 0], [-9, 0, 0], [0, 1, 0], [1, 0, 1]]
    assert rr.farthest_pair(pts) == rr.farthest_pair_literal(pts) == (0, 1, 324.0)
    # ... also when a later pair ties with it
    pts = [[9, 0, 0], [-9, 0, 0], [0, 9, 0], [0, -9, 0]]
    assert rr.farthest_pair(pts) == rr.farthest_pair_literal(pts) == (0, 1, 324.0)
    # a new maximum with a.x > b.x is swapped
    pts = [[0, 0, 0], [1, 0, 0], [5, 0, 0], [-5, 1, 0]]
    assert rr.farthest_pair(pts) == rr.farthest_pair_literal(pts) == (3, 2, 101.0)
    # ... with a.x == b.x not
    pts = [[0, 0, 0], [1, 0, 0], [2, 7, 0], [2, -7, 0]]
    assert rr.farthest_pair(pts) == rr.farthest_pair_literal(pts) == (2, 3, 196.0)
    # of two pairs at the largest distance the first in scan order, though the later has the smaller x
    pts = [[0, 0, 0], [1, 0, 0], [0, 6, 0], [0, -6, 0], [-6, 0, 0], [6, 0, 0]]
    assert rr.farthest_pair(pts) == rr.farthest_pair_literal(pts) == (2, 3, 144.0)


def test_rotation():
    x = rr.X_AXIS
    for v in (x, (-1.0, 0.0, 0.0)):                  # parallel and antiparallel: the identity
        np.testing.assert_array_equal(rr.rotation(v, x), rr.identity())
    v = rr.normalize((0.3, -0.5, 0.81))
    np.testing.assert_array_equal(rr.rotation(v, v), rr.identity())
    np.testing.assert_array_equal(rr.rotation(v, tuple(-c for c in v)), rr.identity())
    rng = np.random.default_rng(5)
    for _ in range(50):
        v0, v1 = rr.normalize(tuple(rng.normal(size=3))), rr.normalize(tuple(rng.normal(size=3)))
        for a, b in ((v0, v1), (v0, x)):
            t = rr.rotation(a, b)
            assert np.all(t[:, 3] == 0.0)
            r = t[:, :3]
            for q in (r, r.T):   # orthonormal: rows and columns of length 1 and at right angles, to 1e-15
                assert max(abs(np.linalg.norm(q[i]) - 1.0) for i in range(3)) <= 1e-15
                assert max(abs(q[i] @ q[j]) for i in range(3) for j in range(i)) <= 1e-15
            assert abs(np.linalg.det(r) - 1.0) <= 1e-14
            assert np.abs(r @ np.array(a) - np.array(b)).max() <= 1e-12
    # beyond acos' domain (a dot product above 1 by an ulp): NaN as Math.acos gives, no exception
    assert np.isnan(rr.rotation((1.0000000000000002, 1e-9, 0.0), x)).sum() == 9
    assert rr.normalize((0.0, 0.0, 0.0))[0] != rr.normalize((0.0, 0.0, 0.0))[0]


def test_math_min_max():
    nan, nz = math.nan, -0.0
    assert math.isnan(rr.java_min(nan, 1.0)) and math.isnan(rr.java_min(1.0, nan))
    assert math.isnan(rr.java_max(nan, 1.0)) and math.isnan(rr.java_max(1.0, nan))
    assert math.copysign(1.0, rr.java_min(0.0, nz)) < 0 and math.copysign(1.0, rr.java_min(nz, 0.0)) < 0
    assert math.copysign(1.0, rr.java_max(0.0, nz)) > 0 and math.copysign(1.0, rr.java_max(nz, 0.0)) > 0
    box = rr.box_of([[1.0, nz, nan], [2.0, 0.0, 3.0]])
    assert box[0] == 1.0 and box[3] == 2.0 and math.isnan(box[2]) and math.isnan(box[5])
    assert math.copysign(1.0, box[1]) < 0 and math.copysign(1.0, box[4]) > 0
    assert rr.size_simple([[1.0, nz, 5.0], [2.0, 0.0, 3.0]]) == ([1.0, nz, 3.0], [2.0, 0.0, 5.0])
    assert math.copysign(1.0, rr.size_simple([[1.0, 0.0, 5.0], [2.0, nz, 3.0]])[0][1]) < 0


def test_optimal_bounding_box_finds_the_cuboid():
    """400 points that fill a 200 x 40 x 20 cuboid (its corners among them), turned so that its
    long axis lies along CUBOID_AXIS.

    The bound.  A box of the corners cannot be smaller than the cuboid itself.  The search ends
    on a grid of spacing 0.001 per component about a unit vector, so where it converges its
    axis v is within eps = sqrt(3) * 0.001 of the cuboid's; the found rotation followed by the
    scene's is then a rotation by at most delta = 2 * eps (x is taken to a vector eps away, and
    the roll that the two minimal rotations leave is of the same order), whose off-diagonal
    entries are at most sin(delta) <= delta.  The extent of a turned cuboid along axis a is
    sum_b |R_ab| e_b <= e_a + delta * (the other two extents), so
        volume <= (200 + 60 delta) (40 + 220 delta) (20 + 240 delta),  delta = 0.002 sqrt(3),
    6.3 % above 160,000."""
    pts, own = rr.cuboid_points()
    res = rr.optimal_bounding_box(pts)
    aabb = rr.volume_of(rr.box_of(pts))
    assert own * (1.0 - 1e-12) <= res["min_volume"] <= aabb
    delta = 0.002 * math.sqrt(3.0)
    bound = (200 + 60 * delta) * (40 + 220 * delta) * (20 + 240 * delta)
    assert bound < 1.07 * own < 0.1 * aabb           # the scene lies diagonally: its own box is 19 x smaller
    assert res["min_volume"] <= bound
    assert res["min_volume"] == rr.volume_of(res["box"]) <= res["start_volume"]
    # the returned transform is the one the box was measured under, and maps the axis onto x
    np.testing.assert_array_equal(rr.box_of(rr.transform_points(res["transform"], pts)), res["box"])
    assert np.abs(res["transform"][:, :3] @ np.array(res["axis"]) - [1, 0, 0]).max() < 1e-12
    assert abs(np.dot(res["axis"], rr.CUBOID_AXIS)) > math.cos(math.sqrt(3.0) * 0.001)
    # the farthest pair is a body diagonal of the cuboid
    assert abs(res["far_d2"] - (200.0 ** 2 + 40.0 ** 2 + 20.0 ** 2)) < 1e-6


def test_padded_box_known_answers():
    # add = max(10, 2, 1) * 0.1 / 2 ... of the extents 200, 40, 20 at 10 %: 10
    assert rr.padded_box([0.0, 0.0, 0.0], [200.0, 40.0, 20.0], 10.0) == ([-10, -10, -10], [210, 50, 30])
    # Math.round: halves go up, also the negative ones (-2.5 -> -2, -3.5 -> -3, 2.5 -> 3)
    assert rr.padded_box([-2.5, -3.5, 2.5], [-2.5, -3.5, 2.5], 0.0) == ([-2, -3, 3], [-2, -3, 3])
    assert rr.padded_box([-1.5, -0.5, 0.5], [8.5, 0.5, 0.5], 0.0) == ([-1, 0, 1], [9, 1, 1])
    # extents 10, 1, 0 at 50 %: add = 2.5; -1.5 - 2.5 = -4, -0.5 - 2.5 = -3, 0.5 - 2.5 = -2
    assert rr.padded_box([-1.5, -0.5, 0.5], [8.5, 0.5, 0.5], 50.0) == ([-4, -3, -2], [11, 3, 3])
    assert rr.padded_box([-0.6, 0.4, 0.49], [-0.6, 0.4, 0.49], 0.0) == ([-1, 0, 0], [-1, 0, 0])
    assert rr.java_int(rr.java_round(math.nan)) == 0 and rr.java_int(2 ** 31) == -2 ** 31


def test_world_points_and_the_whole_step():
    lists, models, corr = rr.cuboid_views()
    pts, _ = rr.cuboid_points()
    w = rr.world_points(lists, models)
    assert w.shape == (400, 3) and np.abs(w - pts).max() < 1e-10           # in view order
    wc = rr.world_points(lists, models, corr)
    o = np.cumsum([0] + [len(p) for p in lists])
    np.testing.assert_array_equal(wc, np.concatenate([w[o[v] + corr[v]] for v in range(3)]))
    np.testing.assert_array_equal(rr.world_points(lists, models, corr, detections="all"), w)
    res = rr.reorient_bounding_box(lists, models, corr, 10.0, True)
    assert res["bb_dims"] == tuple(h - l + 1 for l, h in zip(res["bb_min"], res["bb_max"]))
    under = np.concatenate([rr.transform_points(m, p) for m, p in zip(res["new_models"], lists)])
    assert np.abs(under - rr.transform_points(res["transform"], w)).max() < 1e-9
    simple = rr.reorient_bounding_box(lists, models, None, 0.0, False)
    np.testing.assert_array_equal(simple["transform"], rr.identity())
    assert simple["min_f"] == w.min(axis=0).tolist() and simple["max_f"] == w.max(axis=0).tolist()


# ---------------------------------------------------------------- the library without a GPU
def test_exported_defaults_and_tile(lib):
    p = _lib.ReorientParams()
    lib.spim_reorient_params_default(C.byref(p))
    assert (p.use_corresponding, p.reorientate, p.percent, p.device, p.far_split) == (1, 1, 10.0, 0, 0)
    assert C.sizeof(_lib.ReorientParams) == 56 and C.sizeof(_lib.ReorientResult) == 280
    assert bb.reorient_tile() == 256
    for name in ("farthest_pair", "axis_boxes", "points_min_max", "reorient_bounding_box", "preconcatenate"):
        assert name in bb.__all__


def test_preconcatenate_equals_the_restatement():
    rng = np.random.default_rng(9)
    for _ in range(20):
        t, m = rng.normal(size=(3, 4)), rng.normal(size=(3, 4)) * 100.0
        got = bb.preconcatenate(t, m)
        np.testing.assert_array_equal(got.view(np.uint64), rr.preconcatenate(t, m).view(np.uint64))
        full = lambda a: np.vstack([a, [0, 0, 0, 1.0]])
        assert np.abs(got - (full(t) @ full(m))[:3]).max() < 1e-10
