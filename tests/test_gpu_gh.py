"""GPU parity of the geometric hashing candidate stage (csrc/geohash.hip) against the
restatement in tests/gh_ref.py, bit for bit: neighbours, the six descriptor floats, best_idx /
best / second over every A point, the ordered candidate list; then registration and the
pipeline's ``matching="geometric_hashing"`` on views whose rotations are not known.

Bit for bit: equal uint32 / uint64 views; two NaNs are equal whatever their payload, the sign
of a zero counts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import gh_ref as gr
import rgldm_ref as rr
from spim_registration_amd import _lib, globalopt, pipeline, registration, synthetic

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def pair(seed, na, nb):
    return gr.make_pair(seed, na, nb)


@functools.lru_cache(maxsize=None)
def reference(seed, na, nb):
    """the restatement's result for a pair of PAIR_CASES: computed once, shared, read-only"""
    a, b = pair(seed, na, nb)
    return gr.geometric_hashing(a, b)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.dtype in (np.float32, np.float64) and got.shape == want.shape
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    nan = np.isnan(got) & np.isnan(want)
    np.testing.assert_array_equal(np.where(nan, 0, got.view(u)), np.where(nan, 0, want.view(u)))


def check_match(a, b, want, ratio=10.0, thr=50.0, **kw):
    ia, ib, idx, best, second = registration.gh_candidates(a, b, ratio, thr, return_all=True, **kw)
    np.testing.assert_array_equal(idx, want["best_idx"])
    same_bits(best, want["best"])
    same_bits(second, want["second"])
    assert ia.dtype == ib.dtype == np.int32
    np.testing.assert_array_equal(ia, want["ia"])
    np.testing.assert_array_equal(ib, want["ib"])
    return ia, ib


def check_descriptors(p, want=None):
    nbr_want, desc_want = gr.descriptors(p) if want is None else want
    nbr, desc = registration.gh_descriptors(p)
    assert nbr.dtype == np.int32 and nbr.shape == (len(p), 3)
    np.testing.assert_array_equal(nbr, nbr_want)
    same_bits(desc, desc_want)
    return nbr, desc


def test_tile_sizes_are_the_ones_the_cases_straddle(gpu):
    assert registration.gh_tile_sizes() == (gr.A_TILE, gr.B_TILE)


# ---------------------------------------------------------------- descriptors
@pytest.mark.parametrize("n", [4, 5, 255, 256, 257])
def test_descriptors_at_sizes(gpu, n):
    """4: every other point is a neighbour; one below / at / above the block of 256"""
    p = rr.random_points(900 + n, n)
    rr.assert_no_knn_ties(p, 3)
    _, desc = check_descriptors(p)
    assert np.isfinite(desc).all() and np.abs(desc[:, 1:]).max() > 1.0


def test_descriptors_of_collinear_points(gpu):
    """six points on a line, the cross product exactly 0: n and y are NaN.  Along (1, 1, 1) the
    LU finds no pivot among NaNs (the RuntimeException), along x two rows are (0, NaN, NaN)
    (singular); both leave bx .. cz at +0 and ax in place"""
    t = np.array([0.0, 1.0, 3.0, 7.0, 15.0, 31.0])
    for direction in ([1.0, 1.0, 1.0], [1.0, 0.0, 0.0]):
        p = np.outer(t, direction) + [3.0, 5.0, 9.0]
        _, desc = check_descriptors(p)
        assert np.all(desc[:, 0] > 0) and np.all(desc[:, 1:].view(np.uint32) == 0)


def test_descriptors_with_coincident_points(gpu):
    """two points at one place: for each the other is the nearest (b = 0); and a point whose
    three neighbours all coincide with it: |d| = 0, x = NaN, ax = 0"""
    p = np.array(rr.random_points(931, 40))
    p[17] = p[5]
    check_descriptors(p)
    q = np.concatenate([np.repeat(p[:1], 4, axis=0), p[1:9]])
    _, desc = check_descriptors(q)
    assert np.all(desc[:4] == 0.0)


def test_descriptors_on_a_lattice(gpu):
    """4 x 4 x 4 integer lattice: every neighbour distance tied (lower index first in the
    library and the restatement alike), collinear and coplanar triples"""
    g = np.arange(4.0)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * 3.0
    check_descriptors(p)


def test_descriptors_of_a_coplanar_set(gpu):
    """all points in the plane z = 7: cz is a zero of either sign"""
    p = np.array(rr.random_points(932, 150))
    p[:, 2] = 7.0
    rr.assert_no_knn_ties(p, 3)
    _, desc = check_descriptors(p)
    cz = desc[:, 5]
    assert np.all(cz == 0.0) and np.signbit(cz).any() and not np.signbit(cz).all()


# ---------------------------------------------------------------- matching
@pytest.mark.parametrize("seed,na,nb", [c for c in gr.PAIR_CASES if min(c[1:]) >= 4])
def test_sizes(gpu, seed, na, nb):
    """the minimum 4 x 4, one below / at / above the A tile and the B tile independently,
    one A tile against several B tiles, 257 x 130, and 520 x 1100, where the automatic split
    takes more than one partition (nb beyond one B tile, few A blocks)"""
    a, b = pair(seed, na, nb)
    want = reference(seed, na, nb)
    ia, _ = check_match(a, b, want)
    if min(na, nb) >= 100:
        assert len(ia) > 0
    check_descriptors(a, (want["neighbors_a"], want["desc_a"]))
    check_descriptors(b, (want["neighbors_b"], want["desc_b"]))


@pytest.mark.parametrize("seed,na,nb", [c for c in gr.PAIR_CASES if min(c[1:]) < 4])
def test_below_the_minimum_is_no_error(gpu, seed, na, nb):
    """GeometricHashingPairwise.java:58-65: zero candidates, no error"""
    a, b = pair(seed, na, nb)
    ia, ib = check_match(a, b, reference(seed, na, nb))
    assert len(ia) == len(ib) == 0
    for x, y in ((np.zeros((0, 3)), b), (a, np.zeros((0, 3))), (np.zeros((0, 3)), np.zeros((0, 3)))):
        ia, ib, idx, best, _ = registration.gh_candidates(x, y, return_all=True)
        assert len(ia) == len(ib) == 0 and np.all(idx == -1) and np.all(best == gr.DOUBLE_MAX)


def test_splits_give_identical_output(gpu):
    """b_split 1, 2, 7 and 400 (more than nb: empty partitions) over nb = 333; among the A
    points are some whose two first ranked B fall into one partition and some where they do not"""
    seed, na, nb = gr.SPLIT_CASE
    a, b = pair(seed, na, nb)
    want = reference(seed, na, nb)
    d = gr.descriptor_distances(want["desc_a"], want["desc_b"])
    two = np.argsort(np.sqrt(d).astype(np.float32), axis=1, kind="stable")[:, :2]
    for split in (1, 2, 7, 400):
        if 1 < split < nb:
            part = two // -(-nb // split)
            assert (part[:, 0] == part[:, 1]).any() and (part[:, 0] != part[:, 1]).any()
        check_match(a, b, want, b_split=split)


def test_threshold_is_strict(gpu):
    """difference_threshold at an A point's own best rejects it (best < threshold); the next
    double accepts it"""
    seed, na, nb = 603, 257, 130
    a, b = pair(seed, na, nb)
    base = reference(seed, na, nb)
    i = int(base["ia"][np.argmax(base["best"][base["ia"]])])
    best = float(base["best"][i])
    assert best > 0.0
    for thr, inside in ((best, False), (float(np.nextafter(best, np.inf)), True)):
        want = gr.geometric_hashing(a, b, difference_threshold=thr)
        assert (i in want["ia"]) == inside
        ia, _ = check_match(a, b, want, thr=thr)
        assert (i in ia) == inside


def test_ratio_test_admits_equality(gpu):
    """B holds the same configuration twice, off A by a jitter: second == best > 0.  That is a
    candidate at ratio_of_distance = 1 (best * ratio <= second) and none at the next double"""
    a, b = gr.jittered_twins(*gr.TWIN_CASE)
    n = len(a)
    up = float(np.nextafter(1.0, 2.0))
    one = gr.geometric_hashing(a, b, ratio_of_distance=1.0)
    assert np.array_equal(one["best"], one["second"]) and np.all(one["best"] > 0.0)
    assert np.array_equal(one["best_idx"], np.arange(n))            # the lower copy
    assert np.array_equal(one["ia"], np.nonzero(one["best"] < 50.0)[0]) and len(one["ia"]) > n // 2
    above = gr.geometric_hashing(a, b, ratio_of_distance=up)
    assert len(above["ia"]) == 0
    for split in (0, 2):   # (2: one copy per partition)
        assert len(check_match(a, b, one, ratio=1.0, b_split=split)[0]) == len(one["ia"])
        assert len(check_match(a, b, above, ratio=up, b_split=split)[0]) == 0


def test_exact_zero_passes(gpu):
    """B = A moved by integers (every neighbour - basis difference exact): best == 0.0
    exactly, and 0 * ratio <= second"""
    a, _ = gr.jittered_twins(*gr.TWIN_CASE)
    b = np.array(a) + [5.0, 7.0, -3.0]
    want = gr.geometric_hashing(a, b)
    assert np.all(want["best"] == 0.0) and np.all(want["second"] > 0.0)
    assert np.array_equal(want["ia"], np.arange(len(a))) and np.array_equal(want["ib"], np.arange(len(a)))
    check_match(a, b, want)


def test_equal_float_keys_rank_by_index(gpu):
    """two B descriptors at different double distances with the same float root: the lower
    index is the best although its distance is the larger one (tests/test_gh_cpu.py checks
    the input holds such A points)"""
    a, b = gr.near_twins()
    want = gr.geometric_hashing(a, b)
    assert (want["best"] > want["second"]).any()
    for split in (0, 1, 2, 5):
        check_match(a, b, want, b_split=split)


def test_device_tensors_equal_host_inputs(gpu):
    seed, na, nb = 603, 257, 130
    a, b = pair(seed, na, nb)
    want = reference(seed, na, nb)
    ta, tb = torch.from_numpy(np.array(a)).cuda(), torch.from_numpy(np.array(b)).cuda()
    check_match(ta, tb, want)
    check_match(ta, b, want)
    check_descriptors(ta, (want["neighbors_a"], want["desc_a"]))
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b)   # inputs untouched


def test_non_finite_input_is_an_error(gpu):
    a, b = (np.array(x) for x in pair(603, 257, 130))
    for bad in (np.nan, np.inf, 1e300):   # (1e300 is not finite as the float the kNN metric reads)
        x = a.copy()
        x[256, 2] = bad
        for args in ((x, b), (b, x)):
            with pytest.raises(_lib.SpimDeconError) as e:
                registration.gh_candidates(*args)
            assert e.value.status == -1 and "non-finite" in str(e.value)
        with pytest.raises(_lib.SpimDeconError):
            registration.gh_descriptors(x)
    with pytest.raises(_lib.SpimDeconError):
        registration.gh_descriptors(a[:3])          # a descriptor needs 4 points


def test_small_cap_reports_the_needed_count(gpu, lib):
    seed, na, nb = gr.SPLIT_CASE
    a, b = (np.ascontiguousarray(x) for x in pair(seed, na, nb))
    want = reference(seed, na, nb)
    need = len(want["ia"])
    assert need > 1
    p = _lib.GhParams()
    lib.spim_gh_params_default(C.byref(p))
    idx, best, second = np.empty(na, np.int32), np.empty(na), np.empty(na)
    ia, ib = np.full(na, -7, np.int32), np.full(na, -7, np.int32)
    n = C.c_int64(-1)

    def run(cap):
        return lib.spim_gh_match(a.ctypes.data, na, b.ctypes.data, nb, C.byref(p), idx.ctypes.data,
                                 best.ctypes.data, second.ctypes.data, ia.ctypes.data, ib.ctypes.data, cap,
                                 C.byref(n))
    assert run(need - 1) == -1 and n.value == need and "capacity" in _lib.last_error()
    assert np.all(ia == -7)
    same_bits(best, want["best"])          # written for every A point all the same
    assert run(need) == 0 and n.value == need
    np.testing.assert_array_equal(ia[:need], want["ia"])
    np.testing.assert_array_equal(ib[:need], want["ib"])
    assert np.all(ia[need:] == -7)


# ---------------------------------------------------------------- registration
def test_register_recovers_unknown_rotations(gpu):
    """four point sets rotated 0 / 45 / 90 / 135 degrees about y and shifted, every given model
    the identity: the candidate lists of every pair are the restatement's, so RANSAC and
    GlobalOpt (host, one seed) return exactly the same models, the planted ones to 1e-6"""
    pts, true, given = gr.registration_scene()
    for u in range(4):
        for v in range(u + 1, 4):
            ia, ib = registration.gh_candidates(pts[u], pts[v])
            ra, rb = gr.candidates(pts[u], pts[v])
            assert len(ra) > 20
            np.testing.assert_array_equal(ia, ra)
            np.testing.assert_array_equal(ib, rb)
    got, res = registration.register(pts, given, model="rigid", matching="geometric_hashing")
    want, wres = registration.register(pts, given, model="rigid", matching="geometric_hashing",
                                       candidates=gr.candidates)
    assert res is not None and not res.unaligned and res.failure is None
    for g, w, t in zip(got, want, true):
        np.testing.assert_array_equal(g, w)
        assert np.abs(g - t).max() < 1e-6
    assert res.error == wres.error and res.iterations == wres.iterations


# ---------------------------------------------------------------- pipeline
WORLD = (48, 44, 40)   # the volume of tests/test_gpu_rgldm.py::test_pipeline_matching_rgldm


def test_pipeline_matching_geometric_hashing(gpu):
    """the non-fixed views' models rotated 10 degrees off about y (through the volume's
    centre): matching="geometric_hashing" with refine="rigid" brings their translation back
    to within max_epsilon, the bound of the RGLDM pipeline test.  A descriptor survives only
    where both views detected a bead and the same three neighbours of it (no redundancy, unlike
    RGLDM), so the beads are sparser here (1 / 12^3) than in that test: fewer close pairs that
    one view's anisotropic PSF merges and the view 90 degrees off resolves"""
    views, models = synthetic.make_timepoint_torch(WORLD, WORLD, 4, timepoint=1, config_id=41,
                                                   bead_density=1.0 / 12 ** 3, device="cuda:0")
    true = [np.asarray(m, np.float64).reshape(3, 4) for m in models]
    centre = np.array(WORLD, np.float64) / 2
    off = np.hstack([gr.rot_y(10.0), (centre - gr.rot_y(10.0) @ centre)[:, None]])
    given = [true[0]] + [globalopt.concatenate(off, m) for m in true[1:]]
    assert min(np.linalg.norm(g[:, 3] - t[:, 3]) for g, t in zip(given[1:], true[1:])) > 2.0
    kw = dict(psf_size=(9, 9, 11), iterations=1, refine="rigid")
    res = pipeline.process_timepoint(views, given, (0, 0, 0), WORLD, matching="geometric_hashing", **kw)
    max_epsilon = 5.0
    assert res.globalopt is not None and not res.globalopt.unaligned
    for got, t in zip(res.models, true):
        assert np.linalg.norm(got[:, 3] - t[:, 3]) < max_epsilon
        assert np.abs(got[:, :3] - t[:, :3]).max() < 0.05
