"""GPU parity of the RGLDM candidate stage (csrc/rgldm.hip) against the restatement in
tests/rgldm_ref.py, bit for bit: neighbours, neighbour - basis vectors, best_idx / best /
second over every A point, the ordered candidate list; then registration and the pipeline's
``matching="rgldm"`` against the same host code fed the restatement's candidates."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import rgldm_ref as rr
from spim_registration_amd import _lib, globalopt, pipeline, registration, synthetic

pytestmark = pytest.mark.gpu

A_TILE, B_TILE = 128, 64


@functools.lru_cache(maxsize=None)
def pair(seed, na, nb):
    return rr.make_pair(seed, na, nb)


@functools.lru_cache(maxsize=None)
def reference(seed, na, nb, nn=3, re=1, ratio=3.0, thr=50.0):
    """the restatement's result for a pair of PAIR_CASES: computed once, shared, read-only"""
    a, b = pair(seed, na, nb)
    return rr.rgldm(a, b, nn, re, ratio, thr)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


def check_match(a, b, want, nn=3, re=1, ratio=3.0, thr=50.0, **kw):
    ia, ib, idx, best, second = registration.rgldm_candidates(a, b, nn, re, ratio, thr, return_all=True, **kw)
    np.testing.assert_array_equal(idx, want["best_idx"])
    same_bits(best, want["best"])
    same_bits(second, want["second"])
    assert ia.dtype == ib.dtype == np.int32
    np.testing.assert_array_equal(ia, want["ia"])
    np.testing.assert_array_equal(ib, want["ib"])
    return ia, ib


def check_descriptors(p, nbr_want, rel_want, nn, re):
    nbr, rel = registration.descriptors(p, nn, re)
    np.testing.assert_array_equal(nbr, nbr_want)
    same_bits(rel, rel_want)


def test_tile_sizes_are_the_ones_the_cases_straddle(gpu):
    assert registration.tile_sizes() == (A_TILE, B_TILE)


@pytest.mark.parametrize("seed,na,nb", [c for c in rr.PAIR_CASES if min(c[1:]) >= 5])
def test_sizes(gpu, seed, na, nb):
    """the minimum (every other point a neighbour), one below / at / above the A tile (128)
    and the B tile (64) independently, 257 x 130, one A tile against several B tiles, and a
    size at which the automatic split takes more than one partition"""
    a, b = pair(seed, na, nb)
    want = reference(seed, na, nb)
    ia, _ = check_match(a, b, want)
    if min(na, nb) >= 100:
        assert len(ia) > 0
    check_descriptors(a, want["neighbors_a"], want["rel_a"], 3, 1)
    check_descriptors(b, want["neighbors_b"], want["rel_b"], 3, 1)


@pytest.mark.parametrize("seed,na,nb", [(302, 4, 5), (303, 5, 4), (309, 2, 2)])
def test_below_the_minimum_is_no_error(gpu, seed, na, nb):
    """RGLDMPairwise.java:46-54: zero candidates, no error"""
    a, b = pair(seed, na, nb)
    ia, ib = check_match(a, b, reference(seed, na, nb))
    assert len(ia) == len(ib) == 0
    ia, ib = registration.rgldm_candidates(np.zeros((0, 3)), b)
    assert len(ia) == len(ib) == 0


def test_splits_give_identical_output(gpu):
    """b_split 1, 2 and 7 over nb = 333 (no multiple of 2 or 7); among the A points are some
    whose best and second best B fall into one partition and some where they do not"""
    seed, na, nb = 306, 200, 333
    a, b = pair(seed, na, nb)
    want = reference(seed, na, nb)
    d = rr.descriptor_distances(want["rel_a"], want["rel_b"], 3)
    two = np.argsort(d, axis=1, kind="stable")[:, :2]
    for split in (1, 2, 7):
        if split > 1:
            part = two // -(-nb // split)
            assert (part[:, 0] == part[:, 1]).any() and (part[:, 0] != part[:, 1]).any()
        check_match(a, b, want, b_split=split)
    check_match(a, b, want, b_split=400)   # more partitions than B descriptors: empty ones


@pytest.mark.parametrize("nn,re", [(3, 1), (3, 0), (2, 2), (4, 2), (1, 0)])
def test_parameters(gpu, nn, re):
    seed, na, nb = 307, 150, 140
    a, b = pair(seed, na, nb)
    want = reference(seed, na, nb, nn, re)
    check_match(a, b, want, nn, re)
    check_match(a, b, want, nn, re, b_split=3)
    check_descriptors(a, want["neighbors_a"], want["rel_a"], nn, re)
    # the minimum size for these parameters
    m = nn + re
    check_match(a[:m + 1], b[:m + 1], rr.rgldm(a[:m + 1], b[:m + 1], nn, re), nn, re)


def test_over_limit_is_an_error(gpu):
    a, b = pair(307, 150, 140)
    for nn, re in ((4, 3), (7, 0), (0, 1), (3, -1)):
        with pytest.raises(_lib.SpimDeconError) as e:
            registration.rgldm_candidates(a, b, nn, re)
        assert e.value.status == -1
    with pytest.raises(_lib.SpimDeconError):
        registration.descriptors(a, 4, 3)
    with pytest.raises(_lib.SpimDeconError):
        registration.descriptors(a[:4], 3, 1)   # a descriptor needs nn + re + 1 points


def test_twin_clusters_tie(gpu):
    """B holds the same translated cluster twice: second == best, best_idx the lower copy, and
    the ratio test rejects every point -- also with ratio_of_distance = 1 (strict <)"""
    a, b = rr.twin_clusters(*rr.TWIN_CASE)
    n = len(a)
    for ratio in (3.0, 1.0):
        want = rr.rgldm(a, b, ratio_of_distance=ratio)
        assert np.array_equal(want["best_idx"], np.arange(n)) and np.all(want["best"] == 0.0)
        assert np.all(want["second"] == want["best"]) and len(want["ia"]) == 0
        for split in (0, 1, 2, 3):   # (2: one copy per partition)
            check_match(a, b, want, ratio=ratio, b_split=split)


def test_threshold_is_strict(gpu):
    """one B point moved by 1.5 along x under (3, 0): a descriptor holding it has best ==
    2.25 / 3.0 == 0.75, a float; that threshold rejects it, the next float accepts it"""
    a, _ = rr.twin_clusters(*rr.TWIN_CASE)
    b = np.array(a) + [5.0, 7.0, -3.0]
    b[17, 0] += 1.5
    base = rr.rgldm(a, b, 3, 0)
    hit = np.nonzero((base["best"] == 0.75) & np.isin(np.arange(len(a)), base["ia"]))[0]
    assert len(hit) > 0
    i = int(hit[0])
    up = float(np.nextafter(np.float32(0.75), np.float32(1)))
    for thr, inside in ((0.75, False), (up, True)):
        want = rr.rgldm(a, b, 3, 0, difference_threshold=thr)
        assert (i in want["ia"]) == inside
        ia, _ = check_match(a, b, want, 3, 0, thr=thr)
        assert (i in ia) == inside


def test_device_tensors_equal_host_inputs(gpu):
    seed, na, nb = 304, 257, 130
    a, b = pair(seed, na, nb)
    want = reference(seed, na, nb)
    ta, tb = torch.from_numpy(np.array(a)).cuda(), torch.from_numpy(np.array(b)).cuda()
    check_match(ta, tb, want)
    check_match(ta, b, want)
    check_descriptors(ta, want["neighbors_a"], want["rel_a"], 3, 1)
    same_bits(ta.cpu().numpy(), a)   # inputs untouched
    same_bits(tb.cpu().numpy(), b)


def test_small_cap_reports_the_needed_count(gpu, lib):
    seed, na, nb = 306, 200, 333
    a, b = (np.ascontiguousarray(x) for x in pair(seed, na, nb))
    want = reference(seed, na, nb)
    need = len(want["ia"])
    assert need > 1
    p = _lib.RgldmParams()
    lib.spim_rgldm_params_default(C.byref(p))
    idx, best, second = np.empty(na, np.int32), np.empty(na), np.empty(na)
    ia, ib = np.full(na, -7, np.int32), np.full(na, -7, np.int32)
    n = C.c_int64(-1)

    def run(cap):
        return lib.spim_rgldm_match(a.ctypes.data, na, b.ctypes.data, nb, C.byref(p), idx.ctypes.data,
                                    best.ctypes.data, second.ctypes.data, ia.ctypes.data, ib.ctypes.data, cap,
                                    C.byref(n))
    assert run(need - 1) == -1 and n.value == need and "capacity" in _lib.last_error()
    assert np.all(ia == -7)
    same_bits(best, want["best"])          # written for every A point all the same
    assert run(need) == 0 and n.value == need
    np.testing.assert_array_equal(ia[:need], want["ia"])
    np.testing.assert_array_equal(ib[:need], want["ib"])
    assert np.all(ia[need:] == -7)


def test_non_finite_input_is_an_error(gpu):
    a, b = (np.array(x) for x in pair(307, 150, 140))
    for bad in (np.nan, np.inf, 1e300):   # (1e300 is not finite as the float the kNN metric reads)
        x = a.copy()
        x[149, 2] = bad
        for args in ((x, b), (b, x)):
            with pytest.raises(_lib.SpimDeconError) as e:
                registration.rgldm_candidates(*args)
            assert e.value.status == -1 and "non-finite" in str(e.value)
        with pytest.raises(_lib.SpimDeconError):
            registration.descriptors(x)


# ---------------------------------------------------------------- registration
@pytest.mark.parametrize("kind", ["rigid", "affine"])
def test_register_equals_the_restatement_fed_path(gpu, kind):
    """4 noisy point sets off by 5-30 px: the candidate lists of every pair are the
    restatement's, so RANSAC and GlobalOpt (host, one seed) return exactly the same models"""
    pts, true, given = rr.registration_scene(kind, 0.1)
    world = [globalopt.apply(g, p) for g, p in zip(given, pts)]
    for u in range(4):
        for v in range(u + 1, 4):
            ia, ib = registration.rgldm_candidates(world[u], world[v])
            ra, rb = rr.candidates(world[u], world[v])
            assert len(ra) > 20
            np.testing.assert_array_equal(ia, ra)
            np.testing.assert_array_equal(ib, rb)
    got, res = registration.register(pts, given, model=kind)
    want, wres = registration.register(pts, given, model=kind, candidates=rr.candidates)
    assert res is not None and not res.unaligned
    for g, w, t in zip(got, want, true):
        np.testing.assert_array_equal(g, w)
        assert np.abs(g - t).max() < 0.5          # (noise 0.1 px; the given models are 5-30 px off)
    assert res.error == wres.error and res.iterations == wres.iterations


@pytest.mark.parametrize("kind", ["rigid", "affine"])
def test_register_recovers_planted_models(gpu, kind):
    pts, true, given = rr.registration_scene(kind, 0.0)
    got, res = registration.register(pts, given, model=kind)
    assert res is not None and not res.unaligned and res.failure is None
    for g, t in zip(got, true):
        assert np.abs(g - t).max() < 1e-6


# ---------------------------------------------------------------- pipeline
WORLD = (48, 44, 40)


def test_pipeline_matching_rgldm(gpu):
    """models off by (6, -4, 3) px on the non-fixed views: matching="rgldm" brings their
    translation back to within max_epsilon and equals the restatement-fed path; the default
    "nearest" (2 px radius) cannot"""
    views, models = synthetic.make_timepoint_torch(WORLD, WORLD, 4, timepoint=1, config_id=41,
                                                   bead_density=1.0 / 9 ** 3, device="cuda:0")
    true = [np.asarray(m, np.float64).reshape(3, 4) for m in models]
    shifted = [m.copy() for m in true]
    for m in shifted[1:]:
        m[:, 3] += (6.0, -4.0, 3.0)
    kw = dict(psf_size=(9, 9, 11), iterations=1, refine="translation")
    with pytest.raises(ValueError):
        pipeline.process_timepoint(views, shifted, (0, 0, 0), WORLD, matching="bogus", **kw)
    res = pipeline.process_timepoint(views, shifted, (0, 0, 0), WORLD, matching="rgldm", **kw)
    assert all(len(p) >= 20 for p in res.points)
    want, _ = registration.register(res.points, shifted, model="translation", candidates=rr.candidates)
    max_epsilon = 5.0
    for got, w, t in zip(res.models, want, true):
        np.testing.assert_array_equal(got, w)
        assert np.linalg.norm(got[:, 3] - t[:, 3]) < max_epsilon
    assert res.globalopt is not None and not res.globalopt.unaligned
    near = pipeline.process_timepoint(views, shifted, (0, 0, 0), WORLD, matching="nearest", **kw)
    assert max(np.linalg.norm(g[:, 3] - t[:, 3]) for g, t in zip(near.models, true)) > 2.0
