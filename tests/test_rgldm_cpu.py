"""CPU: the RGLDM restatement (tests/rgldm_ref.py) on planted matches, the host RANSAC of
``registration.ransac``, and the C-ABI's host-side rules (defaults; no GPU, no result)."""
import ctypes as C
import os

import numpy as np
import pytest

import rgldm_ref as rr
from spim_registration_amd import _lib, globalopt, registration


def test_compute_pd():
    assert rr.compute_pd(4, 3) == [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]]
    c = rr.compute_pd(5, 3)
    assert len(c) == 10 and c == sorted(c) and len({tuple(r) for r in c}) == 10
    assert all(r == sorted(r) and 0 <= r[0] and r[-1] <= 4 for r in c)
    assert rr.compute_pd(3, 3) == [[0, 1, 2]]
    assert len(rr.compute_pd(6, 4)) == 15 and len(rr.compute_pd(6, 3)) == 20
    assert rr.compute_pd(3, 2, offset=1) == [[1, 2], [1, 3], [2, 3]]


def test_gpu_test_inputs_have_no_knn_ties():
    """The inputs of tests/test_gpu_rgldm.py, checked here on the CPU for every neighbour
    count up to the maximum."""
    for seed, na, nb in rr.PAIR_CASES:
        for p in rr.make_pair(seed, na, nb):
            if len(p) > 2:
                rr.assert_no_knn_ties(p, 6)
    for p in rr.twin_clusters(*rr.TWIN_CASE):
        rr.assert_no_knn_ties(p, 6)
    for kind in ("rigid", "affine"):
        for noise in (0.0, 0.1):
            pts, _, given = rr.registration_scene(kind, noise)
            for p, g in zip(pts, given):
                rr.assert_no_knn_ties(globalopt.apply(g, p), 4)


@pytest.mark.parametrize("kind", ["rigid", "affine"])
def test_register_recovers_planted_models_from_restated_candidates(kind):
    """The host part of ``register`` (RANSAC, GlobalOpt, concatenate) over the restatement's
    candidates: models off by 5-30 px come back to 1e-6 on noise-free detections."""
    pts, true, given = rr.registration_scene(kind, 0.0)
    got, res = registration.register(pts, given, model=kind, candidates=rr.candidates)
    assert res is not None and not res.unaligned and res.failure is None
    for g, t in zip(got, true):
        assert np.abs(g - t).max() < 1e-6


def test_tie_helper_sees_a_tie():
    p = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 5, 0], [0, 0, 9], [20, 20, 20]], np.float64)
    with pytest.raises(AssertionError):
        rr.assert_no_knn_ties(p, 3)


def test_best_second_vectorised_equals_literal():
    rng = np.random.default_rng(5)
    d = rng.uniform(0, 10, (40, 9))
    d[3, 2] = d[3, 6] = d[3].min() - 1.0        # equal best values: second == best, the lower index
    d[4, :] = rr.DOUBLE_MAX                       # nothing below Double.MAX_VALUE
    d[5, 1] = np.nan
    best, idx, second = rr.best_second(d)
    for i, row in enumerate(d):
        assert (best[i], idx[i], second[i]) == rr.best_second_literal(row)
    assert idx[3] == 2 and best[3] == second[3] and idx[4] == -1


def test_restatement_finds_planted_pairs():
    """B = a shuffled, translated copy of part of A plus unrelated points: the candidates are
    exactly the planted pairs whose neighbourhoods survived, each with best == 0."""
    a = rr.random_points(31, 120)
    rng = np.random.default_rng(32)
    perm = rng.permutation(120)
    # integer-valued translation of coordinates with few mantissa bits: neighbour - basis is exact in both
    a = np.round(np.asarray(a) * 64) / 64
    t = np.array([17.0, -9.0, 4.0])
    extra = np.round(rng.uniform(400, 700, (30, 3)) * 64) / 64      # far from A + t: no shared neighbours
    b = np.concatenate([a[perm] + t, extra])
    rr.assert_no_knn_ties(a, 4)
    rr.assert_no_knn_ties(b, 4)
    r = rr.rgldm(a, b)
    inv = np.argsort(perm)
    # every A point has its translated twin with an identical descriptor
    assert np.array_equal(r["best_idx"], inv.astype(np.int32))
    assert np.all(r["best"] == 0.0) and np.all(r["second"] > 0.0)
    assert np.array_equal(r["ia"], np.arange(120)) and np.array_equal(r["ib"], inv)


def _planted(kind, rng, n=60, outliers=60):
    p = rng.uniform(0, 300, (n + outliers, 3))
    if kind == "translation":
        m = np.hstack([np.eye(3), [[12.0], [-7.0], [21.0]]])
    elif kind == "rigid":
        ax = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
        k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        r = np.eye(3) + np.sin(0.4) * k + (1 - np.cos(0.4)) * k @ k
        m = np.hstack([r, [[5.0], [14.0], [-9.0]]])
    else:
        m = np.hstack([np.eye(3) + rng.uniform(-0.1, 0.1, (3, 3)), [[-11.0], [6.0], [8.0]]])
    q = globalopt.apply(m, p)
    q[n:] += rng.uniform(40, 120, (outliers, 3)) * rng.choice([-1, 1], (outliers, 3))   # 50 % gross outliers
    order = rng.permutation(n + outliers)
    return p[order], q[order], m, np.sort(np.nonzero(order < n)[0])


@pytest.mark.parametrize("kind", ["translation", "rigid", "affine"])
def test_ransac_recovers_planted_model(kind):
    p, q, m, true_inl = _planted(kind, np.random.default_rng(77))
    inl, got, err = registration.ransac(p, q, kind, seed=3)
    assert got is not None and np.abs(got - m).max() < 1e-9
    assert err < 1e-9 and set(inl) <= set(true_inl) and len(inl) >= len(true_inl) // 2
    # deterministic per seed
    inl2, got2, err2 = registration.ransac(p, q, kind, seed=3)
    assert np.array_equal(inl, inl2) and np.array_equal(got, got2) and err == err2


def test_ransac_min_num_correspondences():
    """minNumCorrespondences = max(MIN, round(MIN * factor)) (RANSAC.java:31): fewer candidates
    give no inliers and NaN, whatever they are."""
    rng = np.random.default_rng(9)
    p = rng.uniform(0, 100, (12, 3))
    q = p + [3.0, 4.0, 5.0]
    for kind, least in (("translation", 1), ("rigid", 3), ("affine", 4)):
        need = max(least, int(np.floor(least * 3.0 + 0.5)))
        inl, m, err = registration.ransac(p[:need - 1], q[:need - 1], kind)
        assert len(inl) == 0 and m is None and np.isnan(err)
        inl, m, err = registration.ransac(p[:need], q[:need], kind)
        assert len(inl) == need and np.abs(m[:, 3] - [3, 4, 5]).max() < 1e-9
    inl, m, err = registration.ransac(p[:2], q[:2], "translation", min_inlier_factor=2.5)   # round(2.5) = 3
    assert len(inl) == 0 and np.isnan(err)
    with pytest.raises(ValueError):
        registration.ransac(p, q, "interpolated-affine")


def test_ransac_no_model_among_noise():
    rng = np.random.default_rng(10)
    inl, m, err = registration.ransac(rng.uniform(0, 300, (80, 3)), rng.uniform(0, 300, (80, 3)), "rigid",
                                      max_epsilon=1.0, min_inlier_ratio=0.3)
    assert len(inl) == 0 and m is None and np.isnan(err)


def test_params_default_and_tiles(lib):
    p = _lib.RgldmParams()
    lib.spim_rgldm_params_default(C.byref(p))
    assert (p.num_neighbors, p.redundancy, p.ratio_of_distance, p.difference_threshold) == (3, 1, 3.0, 50.0)
    assert p.b_split == 0 and p.device == 0 and C.sizeof(p) == 24
    a, b = registration.tile_sizes()
    assert a >= 64 and b >= 1


@pytest.mark.skipif(_lib.LIB_PATH.exists() and os.path.exists("/dev/kfd"), reason="GPU visible")
def test_compute_fails_loudly_without_gpu(lib):
    pts = rr.random_points(1, 20)
    with pytest.raises(_lib.SpimDeconError) as e:
        registration.descriptors(pts)
    assert e.value.status == -2 and "no HIP device" in _lib.last_error()
    with pytest.raises(_lib.SpimDeconError) as e:
        registration.rgldm_candidates(pts, pts)
    assert e.value.status == -2 and "no HIP device" in _lib.last_error()
    # the argument rules come first and need no GPU
    with pytest.raises(_lib.SpimDeconError) as e:
        registration.rgldm_candidates(pts, pts, num_neighbors=4, redundancy=3)
    assert e.value.status == -1 and "maximum of 6" in _lib.last_error()
