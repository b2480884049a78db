"""GPU parity of the ICP assignment (csrc/icp.hip) against the restatement in tests/icp_ref.py,
bit for bit: nearest, dist, the ordered match list and the ambiguous count; then the loop,
``register_icp`` and the pipeline's ``icp=True``.

Bit for bit: equal uint32 views of the float distances, equal integers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import icp_ref as ir
from spim_registration_amd import _lib, globalopt, pipeline, registration, synthetic

pytestmark = pytest.mark.gpu

MODELS = {"identity": None, "affine": ir.AFFINE}


@functools.lru_cache(maxsize=None)
def case(seed, nt, nr, model):
    return ir.make_case(seed, nt, nr, MODELS[model])


@functools.lru_cache(maxsize=None)
def reference(seed, nt, nr, model):
    """the restatement's result for a case of SIZE_CASES: computed once, shared, read-only"""
    t, r = case(seed, nt, nr, model)
    return ir.assign(t, r, MODELS[model], return_all=True)


def check_assign(t, r, want, model=None, max_distance=5.0, **kw):
    it, ir_, nearest, dist, ambiguous = registration.icp_assign(t, r, model, max_distance, return_all=True, **kw)
    assert it.dtype == ir_.dtype == nearest.dtype == np.int32 and dist.dtype == np.float32
    np.testing.assert_array_equal(nearest, want[2])
    np.testing.assert_array_equal(dist.view(np.uint32), want[3].view(np.uint32))
    np.testing.assert_array_equal(it, want[0])
    np.testing.assert_array_equal(ir_, want[1])
    assert ambiguous == want[4]
    return it, ir_


def test_tile_sizes_are_the_ones_the_cases_straddle(gpu):
    assert registration.icp_tile_sizes() == (ir.R_BLOCK, ir.T_TILE)


# ---------------------------------------------------------------- assignment
@pytest.mark.parametrize("model", ["identity", "affine"])
@pytest.mark.parametrize("seed,nt,nr", ir.SIZE_CASES)
def test_sizes(gpu, seed, nt, nr, model):
    """the reference list one below / at / above the block, the target list one below / at /
    above the tile, independently; 1 x 1, one target, one reference point; 3112 x 520 and
    2500 x 300, where the automatic split takes more than one partition (tests/test_icp_cpu.py:
    the cases hold matches, non-matches and ambiguous claims)"""
    t, r = case(seed, nt, nr, model)
    check_assign(t, r, reference(seed, nt, nr, model), MODELS[model])


@pytest.mark.parametrize("split", [1, 2, 7, 400])
def test_splits_give_identical_output(gpu, split):
    """t_split 1, 2, 7 and 400 (more than nt = 333 and more than the lattice's 64: empty
    partitions), also where eight targets tie across partitions"""
    seed, nt, nr = ir.SPLIT_CASE
    for model in MODELS:
        check_assign(*case(seed, nt, nr, model), reference(seed, nt, nr, model), MODELS[model], t_split=split)
    for t, r in (ir.lattice_case(), ir.equal_float_case()):
        check_assign(t, r, ir.assign(t, r, return_all=True), t_split=split)


def test_ties_go_to_the_lower_index(gpu):
    """the cell centres of an integer lattice: eight corners at one float distance; and two
    targets at different double distances with the same float distance, the farther one first
    (tests/test_icp_cpu.py checks both inputs are what they say)"""
    t, r = ir.lattice_case()
    want = ir.assign(t, r, return_all=True)
    it, _ = check_assign(t, r, want)
    corner = np.floor(r).astype(int)
    np.testing.assert_array_equal(it, (corner[:, 0] * 4 + corner[:, 1]) * 4 + corner[:, 2])
    t, r = ir.equal_float_case()
    it, _ = check_assign(t, r, ir.assign(t, r, return_all=True))
    np.testing.assert_array_equal(it, 2 * np.arange(len(r)))


def test_threshold_admits_equality(gpu):
    """max_distance exactly a match's float distance keeps it, the next float below drops it"""
    seed, nt, nr = ir.SPLIT_CASE
    t, r = case(seed, nt, nr, "identity")
    base = reference(seed, nt, nr, "identity")
    k = int(base[1][np.argmax(base[3][base[1]])])              # the surviving match that is farthest
    d = base[3][k]
    assert 0.0 < d < 5.0
    for thr, inside in ((float(d), True), (float(np.nextafter(d, np.float32(0.0))), False)):
        assert np.float32(thr) == thr
        want = ir.assign(t, r, max_distance=thr, return_all=True)
        assert (k in want[1]) == inside
        _, ir_ = check_assign(t, r, want, max_distance=thr)
        assert (k in ir_) == inside


def test_ambiguous_matches_are_removed(gpu):
    """two and three reference points on one target: all five go; a claimant beyond the
    threshold claims nothing, the other one of that target stays"""
    t, r, (it, ir_), ambiguous = ir.ambiguity_case()
    want = ir.assign(t, r, return_all=True)
    assert want[4] == ambiguous
    got = check_assign(t, r, want)
    np.testing.assert_array_equal(got[0], it)
    np.testing.assert_array_equal(got[1], ir_)
    for split in (2, 4):
        check_assign(t, r, want, t_split=split)


def test_apply_rounds_every_product_and_sum(gpu):
    """models whose x row casts to another float when a product and a sum are fused
    (tests/test_icp_cpu.py::test_fma_cases_round_differently_when_fused): the distance to the
    origin is the x float of the separately rounded chain"""
    for model, t, r in ir.fma_cases():
        want = ir.assign(t, r, model, return_all=True)
        check_assign(t, r, want, model)
        assert want[3][0] == np.float32(ir.apply(model, t)[0, 0])


def test_device_tensors_equal_host_inputs(gpu):
    seed, nt, nr = ir.SPLIT_CASE
    t, r = case(seed, nt, nr, "affine")
    want = reference(seed, nt, nr, "affine")
    dt, dr = torch.from_numpy(np.array(t)).cuda(), torch.from_numpy(np.array(r)).cuda()
    check_assign(dt, dr, want, ir.AFFINE)
    check_assign(dt, r, want, ir.AFFINE)
    check_assign(t, dr, want, ir.AFFINE)
    assert np.array_equal(dt.cpu().numpy(), t) and np.array_equal(dr.cpu().numpy(), r)   # inputs untouched


def test_non_finite_input_is_an_error(gpu):
    seed, nt, nr = ir.SPLIT_CASE
    t, r = (np.array(x) for x in case(seed, nt, nr, "identity"))
    for bad in (np.nan, np.inf, 1e300):   # (1e300 is not finite as the float Detection.get returns)
        x = t.copy()
        x[256, 2] = bad
        for args in ((x, r), (r, x)):
            with pytest.raises(_lib.SpimDeconError) as e:
                registration.icp_assign(*args)
            assert e.value.status == -1 and "non-finite" in str(e.value)
    big = np.array([[1e37, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])   # 1e37 * x: beyond the float range
    with np.errstate(over="ignore"):
        assert np.isfinite(ir.apply(big, t)).all() and not np.isfinite(ir.apply(big, t).astype(np.float32)).all()
    with pytest.raises(_lib.SpimDeconError) as e:
        registration.icp_assign(t, r, big)
    assert e.value.status == -1 and "non-finite" in str(e.value)
    check_assign(t, r, reference(seed, nt, nr, "identity"))    # the next call is not affected


def test_small_cap_reports_the_needed_count(gpu, lib):
    seed, nt, nr = ir.SPLIT_CASE
    t, r = (np.ascontiguousarray(x) for x in case(seed, nt, nr, "identity"))
    want = reference(seed, nt, nr, "identity")
    need = len(want[0])
    assert need > 1
    p = _lib.IcpParams()
    lib.spim_icp_params_default(C.byref(p))
    nearest, dist = np.empty(nr, np.int32), np.empty(nr, np.float32)
    mt, mr = np.full(nr, -7, np.int32), np.full(nr, -7, np.int32)
    n, amb = C.c_int64(-1), C.c_int64(-1)

    def run(cap):
        return lib.spim_icp_assign(t.ctypes.data, nt, r.ctypes.data, nr, None, C.byref(p), nearest.ctypes.data,
                                   dist.ctypes.data, mt.ctypes.data, mr.ctypes.data, cap, C.byref(n), C.byref(amb))
    assert run(need - 1) == -1 and n.value == need and "capacity" in _lib.last_error()
    assert np.all(mt == -7) and amb.value == want[4]
    np.testing.assert_array_equal(nearest, want[2])            # written for every reference point all the same
    assert run(need) == 0 and n.value == need
    np.testing.assert_array_equal(mt[:need], want[0])
    np.testing.assert_array_equal(mr[:need], want[1])
    assert np.all(mt[need:] == -7)


def test_empty_lists_are_no_error(gpu):
    t, r = case(901, 1, 1, "identity")
    none = np.zeros((0, 3))
    it, ir_, nearest, dist, ambiguous = registration.icp_assign(none, np.repeat(r, 5, axis=0), return_all=True)
    assert len(it) == len(ir_) == 0 and ambiguous == 0
    assert np.all(nearest == -1) and np.all(dist == ir.FLOAT_MAX) and len(dist) == 5
    for args in ((t, none), (none, none)):
        it, ir_, nearest, dist, ambiguous = registration.icp_assign(*args, return_all=True)
        assert len(it) == len(ir_) == len(nearest) == len(dist) == 0 and ambiguous == 0


# ---------------------------------------------------------------- the loop, registration
def test_icp_equals_the_restatement_fed_loop(gpu):
    """the recovery case of tests/test_icp_cpu.py and the one that needs several iterations: the
    loop and the fits are the same host code, so with equal assignments everything is equal"""
    for motion in (ir.RECOVERY_MOTION, ir.FAR_MOTION):
        a, b = ir.recovery_case(motion=motion)
        got = registration.icp(a, b, "rigid")
        want = registration.icp(a, b, "rigid", assign=ir.assign)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2].view(np.uint64), want[2].view(np.uint64))
        assert got[3] == want[3] and got[4] == want[4] and len(got[0]) > 120
        assert np.abs(got[2][:, 3] - motion[:, 3]).max() < 0.05


def test_register_icp_brings_the_views_back(gpu):
    """four views of one bead set, the given models off by up to 1 degree and 2 px: back to
    1e-2 in translation, with more matches per pair than RGLDM returns inliers"""
    pts, true, given = ir.registration_scene()
    got, res = registration.register_icp(pts, given, model="rigid")
    assert res is not None and not res.unaligned and res.failure is None
    for g, t, g0 in zip(got, true, given):
        assert np.abs(g[:, 3] - t[:, 3]).max() < 1e-2
    assert min(np.linalg.norm(g0[:, 3] - t[:, 3]) for g0, t in zip(given[1:], true[1:])) > 1.0
    icp_matches = {(m.a, m.b): len(m.pa) for m in registration.pairwise_icp(pts, given, model="rigid")}
    rgldm = {(m.a, m.b): len(m.pa) for m in registration.pairwise_rgldm(pts, given, model="rigid")}
    assert len(icp_matches) == 6 and set(rgldm) == set(icp_matches)
    for pair, n in rgldm.items():
        assert icp_matches[pair] > n > 0


# ---------------------------------------------------------------- pipeline
WORLD = (48, 44, 40)   # the volume of tests/test_gpu_rgldm.py::test_pipeline_matching_rgldm


def test_pipeline_icp_after_rgldm(gpu):
    """the scene of that test (models off by (6, -4, 3) px): matching="rgldm", refine="affine"
    with icp=True ends within its bound, max_epsilon, with at least as many correspondences as
    without; icp=False changes nothing; icp without refine is an error"""
    views, models = synthetic.make_timepoint_torch(WORLD, WORLD, 4, timepoint=1, config_id=41,
                                                   bead_density=1.0 / 9 ** 3, device="cuda:0")
    true = [np.asarray(m, np.float64).reshape(3, 4) for m in models]
    shifted = [m.copy() for m in true]
    for m in shifted[1:]:
        m[:, 3] += (6.0, -4.0, 3.0)
    kw = dict(psf_size=(9, 9, 11), iterations=1, refine="affine", matching="rgldm", digest=True)
    with pytest.raises(ValueError):
        pipeline.process_timepoint(views, shifted, (0, 0, 0), WORLD, icp=True, **{**kw, "refine": None})
    plain = pipeline.process_timepoint(views, shifted, (0, 0, 0), WORLD, **kw)
    off = pipeline.process_timepoint(views, shifted, (0, 0, 0), WORLD, icp=False, **kw)
    assert off.stage_digests == plain.stage_digests and len(plain.stage_digests) == 3
    for a, b in zip(off.models, plain.models):
        np.testing.assert_array_equal(a, b)
    res = pipeline.process_timepoint(views, shifted, (0, 0, 0), WORLD, icp=True, **kw)
    max_epsilon = 5.0
    assert res.globalopt is not None and not res.globalopt.unaligned
    for got, t in zip(res.models, true):
        assert np.linalg.norm(got[:, 3] - t[:, 3]) < max_epsilon
    assert sum(len(c) for c in res.corresponding) >= sum(len(c) for c in plain.corresponding) > 0
    want, wres = registration.register_icp(res.points, plain.models, model="affine")
    for got, w in zip(res.models, want):
        np.testing.assert_array_equal(got, w)
    assert res.globalopt.error == wres.error
