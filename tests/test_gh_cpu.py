"""CPU: the geometric hashing restatement (tests/gh_ref.py) -- its matrix inversion against
numpy, the rotation invariance of its descriptors, planted rotations recovered through
``registration.pairwise_geometric_hashing`` where RGLDM finds nothing -- and the C-ABI's
host-side rules (defaults, tiles; no GPU, no result)."""
import ctypes as C
import os

import numpy as np
import pytest

import gh_ref as gr
import rgldm_ref as rr
from spim_registration_amd import _lib, globalopt, registration

IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


# ---------------------------------------------------------------- Matrix3d.invert
def test_inversion_agrees_with_numpy():
    rng = np.random.default_rng(11)
    for _ in range(1000):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))          # orthonormal columns
        got = np.array(gr.invert_general(q.reshape(-1))).reshape(3, 3)
        want = np.linalg.inv(q)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_inversion_takes_the_singular_exit():
    rank2 = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 0.0, 1.0]])
    with pytest.raises(gr.SingularMatrixException):
        gr.invert_general(rank2.reshape(-1))
    with pytest.raises(gr.SingularMatrixException):           # Math.abs(NaN) > big is false: big stays 0
        gr.invert_general(np.full(9, np.nan))
    with pytest.raises(gr.SingularMatrixException):
        gr.invert_general(np.zeros(9))
    # one finite column, the others NaN (a collinear triple): no pivot, the RuntimeException,
    # which buildLocalCoordinateSystem's catch ( Exception e ) treats like a singular matrix
    with pytest.raises(RuntimeError):
        gr.invert_general(np.array([0.48, np.nan, np.nan, 0.6, np.nan, np.nan, 0.64, np.nan, np.nan]))
    # collinear triples whose cross product is exactly 0: along (1, 1, 1) the RuntimeException,
    # along x (rows of 0, NaN, NaN) the singular exit; either way bx .. cz = +0 and ax stays
    for x in ([1.0, 1.0, 1.0], [1.0, 0.0, 0.0]):
        d = gr.build_local_coordinate_system(np.outer([1.0, 2.0, 4.0], x))
        assert d[0] == np.float32(4.0 * np.sqrt(np.sum(np.square(x))))
        assert np.all(d[1:] == 0.0) and not np.signbit(d[1:]).any()


def test_inversion_pivots():
    """a matrix whose largest scaled pivot is not on the diagonal: row exchanges in both columns"""
    m = np.array([[0.0, 0.0, 2.0], [3.0, 1.0, 0.0], [0.5, 4.0, 1.0]])
    got = np.array(gr.invert_general(m.reshape(-1))).reshape(3, 3)
    assert np.abs(got @ m - np.eye(3)).max() < 1e-15


def test_vectorised_distance_equals_literal():
    rng = np.random.default_rng(12)
    da = rng.normal(0, 20, (7, 6)).astype(np.float32)
    db = rng.normal(0, 20, (9, 6)).astype(np.float32)
    db[3] = da[2]
    db[4, 1] = np.nan
    d = gr.descriptor_distances(da, db)
    for i in range(7):
        for j in range(9):
            want = gr.descriptor_distance(da[i], db[j])
            assert d[i, j].tobytes() == want.tobytes() or (np.isnan(d[i, j]) and np.isnan(want))
    assert d[2, 3] == 0.0 and np.isnan(d[:, 4]).all()


def test_ranking_rule():
    row = np.array([4.0, np.nan, 1.0, 9.0, 1.0])
    assert gr.rank_two(row) == (1.0, 2, 1.0)                                 # equal keys: lower index first
    assert gr.rank_two(np.array([np.nan, 3.0, np.nan])) == (gr.DOUBLE_MAX, -1, gr.DOUBLE_MAX)
    one = np.nextafter(1.0, 2.0)                                            # the same float root as 1.0
    assert gr.rank_two(np.array([5.0, one, 1.0])) == (one, 1, 1.0)          # ... so best > second
    assert gr.rank_two(np.array([np.inf, 2.0])) == (2.0, 1, np.inf)         # an infinite distance is ranked


# ---------------------------------------------------------------- invariance
def _gapped_points(seed, n, grid=None):
    p = np.random.default_rng(seed).uniform(0.0, 300.0, (n, 3))
    if grid:
        p = np.round(p * grid) / grid
    d = rr.knn_distances(p).astype(np.float64)
    np.fill_diagonal(d, np.inf)
    s = np.sort(d, axis=1)[:, :4]
    assert np.diff(s, axis=1).min() > 1e-3, "kNN distance gaps too small for the invariance test"
    return p


def test_descriptors_are_invariant_under_rigid_motion():
    p = _gapped_points(20, 200)
    rng = np.random.default_rng(22)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))                            # a proper rotation
    moved = p @ q.T + rng.uniform(-50, 50, 3)
    nbr, desc = gr.descriptors(p)
    nbr2, desc2 = gr.descriptors(moved)
    np.testing.assert_array_equal(nbr, nbr2)
    ulp = np.spacing(desc[:, 0]).astype(np.float64)           # one float32 ulp of ax
    diff = np.abs(desc.astype(np.float64) - desc2.astype(np.float64))
    assert np.all(diff <= ulp[:, None])
    assert np.abs(desc[:, 1:]).max() > 1.0                     # (not the all-zero singular exit)


def test_descriptors_keep_every_bit_under_integer_translation():
    p = _gapped_points(23, 200, grid=64)
    nbr, desc = gr.descriptors(p)
    nbr2, desc2 = gr.descriptors(p + np.array([41.0, -17.0, 256.0]))
    np.testing.assert_array_equal(nbr, nbr2)
    np.testing.assert_array_equal(desc.view(np.uint32), desc2.view(np.uint32))


# ---------------------------------------------------------------- planted models
def _planted(seed, angle, n=200):
    """B = A rotated about y and shifted, 50 % unrelated points added to each list, shuffled"""
    rng = np.random.default_rng(seed)
    a_in = rng.uniform(0.0, 300.0, (n, 3))
    m = np.hstack([gr.rot_y(angle), [[17.0], [-9.0], [31.0]]])
    a = np.concatenate([a_in, rng.uniform(0.0, 300.0, (n // 2, 3))])
    b = np.concatenate([globalopt.apply(m, a_in), rng.uniform(-200.0, 500.0, (n // 2, 3))])
    return a[rng.permutation(len(a))], b[rng.permutation(len(b))], m


@pytest.mark.parametrize("angle", [30.0, 90.0, 135.0])
def test_planted_rotation_is_recovered_where_rgldm_finds_nothing(angle):
    a, b, m = _planted(800, angle)
    for kind in ("rigid", "affine"):
        out = registration.pairwise_geometric_hashing([a, b], [IDENTITY, IDENTITY], model=kind,
                                                      candidates=gr.candidates)
        assert len(out) == 1 and len(out[0].pa) >= 20
        fit = globalopt.fit(kind, out[0].pa, out[0].pb, np.ones(len(out[0].pa)))
        assert np.abs(fit - m).max() < 1e-9
        # the translation invariant matcher through the same RANSAC: no pair
        assert registration.pairwise_rgldm([a, b], [IDENTITY, IDENTITY], model=kind, candidates=rr.candidates) == []


def test_too_few_points_give_no_candidates():
    a, b, _ = _planted(800, 30.0, n=20)
    for pa, pb in ((a[:3], b), (a, b[:3]), (a[:0], b), (a, b[:0]), (a[:0], b[:0])):
        r = gr.geometric_hashing(pa, pb)
        assert len(r["ia"]) == len(r["ib"]) == 0 and len(r["best"]) == len(pa)
        assert np.all(r["best_idx"] == -1) and np.all(r["best"] == gr.DOUBLE_MAX)
        assert registration.pairwise_geometric_hashing([pa, pb], [IDENTITY, IDENTITY], model="rigid",
                                                       candidates=gr.candidates) == []


def test_register_rejects_an_unknown_matcher():
    with pytest.raises(ValueError):
        registration.register([np.zeros((5, 3))] * 2, [IDENTITY] * 2, matching="icp")


# ---------------------------------------------------------------- the GPU tests' inputs
def test_gpu_test_inputs_have_no_knn_ties():
    for seed, na, nb in gr.PAIR_CASES:
        for p in gr.make_pair(seed, na, nb):
            if len(p) > 4:
                rr.assert_no_knn_ties(p, 3)
    for p in gr.jittered_twins(*gr.TWIN_CASE) + gr.near_twins():
        rr.assert_no_knn_ties(p, 3)
    for p in gr.registration_scene()[0]:
        rr.assert_no_knn_ties(p, 3)


def test_near_twins_hold_the_tie_the_ranking_rule_decides():
    a, b = gr.near_twins()
    r = gr.geometric_hashing(a, b)
    n = len(a)
    d = gr.descriptor_distances(r["desc_a"], r["desc_b"])
    lo = r["best_idx"] % n
    d1, d2 = d[np.arange(n), lo], d[np.arange(n), lo + n]
    tie = (np.sqrt(d1).astype(np.float32) == np.sqrt(d2).astype(np.float32)) & (d1 != d2)
    assert tie.any()
    # ... among them A points whose lower-index copy is the farther one in double: it still ranks first
    inverted = tie & (d1 > d2)
    assert inverted.any()
    assert np.all(r["best_idx"][inverted] == lo[inverted]) and np.all(r["best"][inverted] > r["second"][inverted])


# ---------------------------------------------------------------- C ABI, host side
def test_params_default_and_tiles(lib):
    p = _lib.GhParams()
    lib.spim_gh_params_default(C.byref(p))
    assert (p.ratio_of_distance, p.difference_threshold, p.b_split, p.device) == (10.0, 50.0, 0, 0)
    assert C.sizeof(p) == 24
    assert registration.gh_tile_sizes() == (gr.A_TILE, gr.B_TILE)


@pytest.mark.skipif(_lib.LIB_PATH.exists() and os.path.exists("/dev/kfd"), reason="GPU visible")
def test_compute_fails_loudly_without_gpu(lib):
    pts = rr.random_points(1, 20)
    with pytest.raises(_lib.SpimDeconError) as e:
        registration.gh_descriptors(pts)
    assert e.value.status == -2 and "no HIP device" in _lib.last_error()
    with pytest.raises(_lib.SpimDeconError) as e:
        registration.gh_candidates(pts, pts)
    assert e.value.status == -2 and "no HIP device" in _lib.last_error()
    # the argument rules come first and need no GPU
    with pytest.raises(_lib.SpimDeconError) as e:
        registration.gh_descriptors(pts[:3])
    assert e.value.status == -1 and "needs 4 points" in _lib.last_error()
    with pytest.raises(_lib.SpimDeconError) as e:
        registration.gh_candidates(pts, pts, b_split=-1)
    assert e.value.status == -1 and "b_split" in _lib.last_error()
