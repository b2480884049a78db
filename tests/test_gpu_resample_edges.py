"""The resampling kernels of csrc/input_prep.hip (k_transform_view, k_weight_sum,
k_final_weight, k_fuse) and csrc/resample.hpp at their edges: tile geometry, portion
arithmetic of the overlap statistics, the grid-stride path, 1- and 2-thick sources, an
analytic ramp that does not go through the oracle, realistic world coordinates, 1 and 7
views, device-resident buffers and argument errors.  The cases are built in
tests/resample_cases.py; tests/test_resample_premises_cpu.py proves on the oracle that
each has the property its test here relies on (P1-P6).

Tolerances are the project's: images through assert_mismatches_on_ties (rtol 1e-5, 4-ulp
tie window, < 1e-3 of the voxels), weights rtol 1e-5 / atol 1e-6; everything that is an
integer or the same float arithmetic is compared exactly."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch  # before the library loads (one shared HIP runtime, spim_registration_amd._lib.load)

import resample_cases as rc
from oracle import fusion_ref as fr
from oracle import input_ref as ir
from spim_registration_amd import _lib
from spim_registration_amd.input_prep import WeightType, fuse_weighted_average, prepare_inputs
from test_gpu_input_prep import assert_mismatches_on_ties

pytestmark = pytest.mark.gpu

SPIMDECON_ERR_ARG = -1   # include/spimdecon.h
WEIGHTED = [WeightType.PRECOMPUTED_WEIGHTS, WeightType.VIRTUAL_WEIGHTS]


def assert_weights_close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


def fuse_raw(srcs, models, bb_min, bb_dims, ds=1.0, interp=1, blend=True, borders=None, ranges=None,
             sigmas=None, on_device=False):
    """spim_fuse_weighted_average(_content) through ctypes with FusionParams filled as
    input_prep.fuse_weighted_average does, plus src_on_device / out_on_device (which
    the Python wrapper never sets).  Returns (status, fused [z, y, x] numpy)."""
    lib = _lib.load()
    V = len(srcs)
    shape = (int(bb_dims[2]), int(bb_dims[1]), int(bb_dims[0]))
    srcs = [np.ascontiguousarray(s, np.float32) for s in srcs]
    if on_device:
        dsrc = [torch.from_numpy(s).cuda() for s in srcs]
        dout = torch.full(shape, -1.0, dtype=torch.float32, device="cuda")
        ptrs = [C.cast(C.c_void_p(t.data_ptr()), _lib._pf) for t in dsrc]
        outp = C.cast(C.c_void_p(dout.data_ptr()), _lib._pf)
    else:
        out = np.full(shape, -1.0, np.float32)
        ptrs = [_lib.fptr(s) for s in srcs]
        outp = _lib.fptr(out) if out.size else None
    views = (_lib.ViewSource * V)()
    for v, (s, m) in enumerate(zip(srcs, models)):
        views[v].img = ptrs[v]
        views[v].dims[:] = [s.shape[2], s.shape[1], s.shape[0]]
        views[v].model[:] = [float(x) for x in np.asarray(m, np.float64).reshape(12)]
    p = _lib.FusionParams()
    lib.spim_fusion_params_default(C.byref(p))
    p.bb_min[:] = [int(x) for x in bb_min]
    p.bb_dims[:] = [int(x) for x in bb_dims]
    p.downsampling = float(ds)
    p.interpolation = int(interp)
    p.use_blending = int(bool(blend))
    p.src_on_device = p.out_on_device = int(on_device)
    b = None if borders is None else np.ascontiguousarray(np.asarray(borders, np.float32).reshape(V, 3))
    r = None if ranges is None else np.ascontiguousarray(np.asarray(ranges, np.float32).reshape(V, 3))
    bp, rp = (None if b is None else _lib.fptr(b)), (None if r is None else _lib.fptr(r))
    if on_device:
        torch.cuda.synchronize()   # the library runs on its own stream
    if sigmas is None:
        status = lib.spim_fuse_weighted_average(V, views, C.byref(p), bp, rp, outp)
    else:
        s1 = np.ascontiguousarray(np.tile(np.asarray(sigmas[0], np.float64), (V, 1)))
        s2 = np.ascontiguousarray(np.tile(np.asarray(sigmas[1], np.float64), (V, 1)))
        status = lib.spim_fuse_weighted_average_content(V, views, C.byref(p), bp, rp, s1.ctypes.data_as(_lib._pd),
                                                        s2.ctypes.data_as(_lib._pd), outp)
    if on_device:
        torch.cuda.synchronize()
        out = dout.cpu().numpy()
    return status, out


# ---------------------------------------------------------------- 1. crop invariance
@functools.lru_cache(maxsize=None)
def _crop_enclosing():
    srcs, models, b0, bd = rc.crop_case()
    imgs, ws, _ = prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, WeightType.NO_WEIGHTS)
    fused = fuse_weighted_average(srcs, models, b0, bd, 1.0, 1, True, rc.CROP_FUSE_BORDERS, rc.CROP_FUSE_RANGES)
    return imgs, ws, fused


def test_crop_enclosing_box_matches_oracle(gpu):
    srcs, models, b0, bd = rc.crop_case()
    imgs, ws, fused = _crop_enclosing()
    ei, ew, _ = ir.prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, ir.NO_WEIGHTS)
    for v in range(len(srcs)):
        assert_mismatches_on_ties(imgs[v], ei[v], [models[v]], b0, bd)
        np.testing.assert_array_equal(ws[v], ew[v])
        assert (imgs[v] > 0).any() and (imgs[v] == 0).any()
    want = fr.fuse_weighted_average(srcs, models, b0, bd, 1.0, 1, True, rc.CROP_FUSE_BORDERS, rc.CROP_FUSE_RANGES)
    assert_mismatches_on_ties(fused, want, models, b0, bd)


@pytest.mark.parametrize("off,dims", rc.CROP_BOXES, ids=lambda v: "x".join(map(str, v)))
def test_prepare_inputs_is_crop_invariant(gpu, off, dims):
    """A voxel's value does not depend on the box it is computed in: float(x) + float(bx)
    is exact for these integers, so every sub-box equals the enclosing box's slice bit
    for bit, whatever part of a 32 x 8 (x, z) tile it fills."""
    srcs, models, b0, _ = rc.crop_case()
    imgs, ws, _ = _crop_enclosing()
    gi, gw, _ = prepare_inputs(srcs, models, rc.sub_box(b0, off), dims, rc.BORDER, rc.RANGE, WeightType.NO_WEIGHTS)
    for v in range(len(srcs)):
        np.testing.assert_array_equal(gi[v], rc.crop(imgs[v], off, dims))
        np.testing.assert_array_equal(gw[v], rc.crop(ws[v], off, dims))


@pytest.mark.parametrize("off,dims", rc.CROP_FUSE_BOXES, ids=lambda v: "x".join(map(str, v)))
def test_fusion_is_crop_invariant(gpu, off, dims):
    srcs, models, b0, _ = rc.crop_case()
    fused = _crop_enclosing()[2]
    got = fuse_weighted_average(srcs, models, rc.sub_box(b0, off), dims, 1.0, 1, True, rc.CROP_FUSE_BORDERS,
                                rc.CROP_FUSE_RANGES)
    np.testing.assert_array_equal(got, rc.crop(fused, off, dims))
    assert (got > 0).any()


# ---------------------------------------------------------------- 2. overlap statistics
def assert_overlap_stats(info, mn, av, ij_threads):
    """min_overlap exactly; avg_overlap within 2 np 2^-52 relative (np = 2 T portions):
    the counts are integers and each per-portion mean is the same double division, only
    the order of the final sum of np doubles differs."""
    assert info["min_overlap"] == mn
    print("avg_overlap", info["avg_overlap"], av)
    if math.isnan(av):
        assert math.isnan(info["avg_overlap"])
    else:
        assert abs(info["avg_overlap"] - av) <= 2 * (2 * ij_threads) * 2.0 ** -52 * abs(av)


@pytest.mark.parametrize("wt", WEIGHTED)
@pytest.mark.parametrize("T", rc.STATS_THREADS)
def test_overlap_statistics_match_oracle(gpu, T, wt):
    """n = 33263 is no multiple of 2 T and the last portion, which takes the remainder,
    sees fewer views than the rest (P2): the per-portion lengths and bounds decide
    avg_overlap.  osem_index 1 / 2 turn the statistics into the OSEM factor."""
    srcs, models, b0, bd = rc.stats_case()
    for osem_index in (0, 1, 2):
        ew, mn, av, eo = rc.expected_weights("stats", int(wt), T, osem_index, 1.0)
        _, ws, info = prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, wt, osem_index, 1.0, ij_threads=T)
        assert_overlap_stats(info, mn, av, T)
        if osem_index == 1:
            assert info["osem"] == float(max(1, mn)) == eo
        elif osem_index == 2:
            assert eo > 1.0 and abs(info["osem"] - eo) <= 2 * (2 * T) * 2.0 ** -52 * eo
        else:
            assert info["osem"] == 1.0
        for v in range(len(srcs)):
            assert_weights_close(ws[v], ew[v])


@pytest.mark.parametrize("wt", WEIGHTED)
def test_fewer_voxels_than_portions(gpu, wt):
    """A 3 x 2 x 2 box with 16 portions: chunk = 0, fifteen empty portions whose mean is
    0 / 0, the last one takes all 12 voxels.  avg_overlap is NaN in the reference too;
    the OSEM factor of index 2 is 1 here and in the oracle."""
    srcs, models, b0, bd = rc.CASES["tiny"]()
    for osem_index in (0, 2):
        ew, mn, av, eo = rc.expected_weights("tiny", int(wt), 8, osem_index, 1.0)
        _, ws, info = prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, wt, osem_index, 1.0, ij_threads=8)
        assert math.isnan(av)
        assert_overlap_stats(info, mn, av, 8)
        assert info["osem"] == eo == 1.0
        for v in range(len(srcs)):
            assert_weights_close(ws[v], ew[v])
            assert (ws[v] > 0).any()


# ---------------------------------------------------------------- 3. grid-stride path
@pytest.mark.parametrize("wt,T", [(WeightType.VIRTUAL_WEIGHTS, 8), (WeightType.VIRTUAL_WEIGHTS, 64),
                                  (WeightType.PRECOMPUTED_WEIGHTS, 8)])
def test_weight_sum_grid_stride(gpu, wt, T):
    """n = 2,244,471 > 8192 * 256: the x grid of k_weight_sum is capped and every thread
    strides over more than one voxel of its portion (P5).  Weights and statistics over
    the whole box against the oracle built from the positions alone."""
    srcs, models, b0, bd = rc.stride_case()
    ew, mn, av, _ = rc.expected_weights("stride", int(wt), T)
    imgs, ws, info = prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, wt, ij_threads=T)
    assert_overlap_stats(info, mn, av, T)
    for v in range(len(srcs)):
        if wt == WeightType.PRECOMPUTED_WEIGHTS:
            nan = np.isnan(ew[v])
            assert nan.any() and not nan.all()
            np.testing.assert_array_equal(np.isnan(ws[v]), nan)
        assert_weights_close(ws[v], ew[v])
    sb = rc.sub_box(b0, rc.STRIDE_SUB_OFF)
    for v in range(len(srcs)):
        ei, _ = ir.transform_view(srcs[v], models[v], sb, rc.STRIDE_SUB_DIMS, rc.BORDER, rc.RANGE, ir.NO_WEIGHTS)
        assert (ei > 0).any()
        assert_mismatches_on_ties(rc.crop(imgs[v], rc.STRIDE_SUB_OFF, rc.STRIDE_SUB_DIMS), ei, [models[v]], sb,
                                  rc.STRIDE_SUB_DIMS)


# ---------------------------------------------------------------- 4. degenerate sources
@pytest.mark.parametrize("wt", list(WeightType))
@pytest.mark.parametrize("dims", rc.DEGENERATE_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_degenerate_sources_prepare_inputs(gpu, dims, wt):
    """1- and 2-thick sources: mirror1's n == 1 branch, and the band t in (s - 1, s) where
    the upper corner mirrors back (P3), on every axis."""
    srcs, models, b0, bd = rc.degenerate_case(dims)
    imgs, ws, info = prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, wt)
    ei, ew, _ = ir.prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, int(wt))
    for v in range(len(srcs)):
        assert_mismatches_on_ties(imgs[v], ei[v], [models[v]], b0, bd)
        assert_weights_close(ws[v], ew[v])
        assert (ei[v] > 0).any() and (ei[v] == 0).any()
    if wt != WeightType.NO_WEIGHTS:
        _, _, mn, av = ir.normalize_weights(list(ir.transform_view(s, m, b0, bd, rc.BORDER, rc.RANGE, int(wt))[1]
                                                 for s, m in zip(srcs, models)), int(wt), 8)
        assert_overlap_stats(info, mn, av, 8)


@pytest.mark.parametrize("interp", [1, 0])
@pytest.mark.parametrize("dims", rc.DEGENERATE_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_degenerate_sources_fusion(gpu, dims, interp):
    srcs, models, b0, bd = rc.degenerate_case(dims)
    b, r = rc.DEGENERATE_FUSE_BORDERS, rc.DEGENERATE_FUSE_RANGES
    got = fuse_weighted_average(srcs, models, b0, bd, 1.0, interp, True, b, r)
    want = fr.fuse_weighted_average(srcs, models, b0, bd, 1.0, interp, True, b, r)
    assert_mismatches_on_ties(got, want, models, b0, bd, half=(interp == 0))
    assert (want > 0).any() and (want == 0).any()


# ---------------------------------------------------------------- 5. analytic ramp
def assert_ramp(got, m, bb_min, bb_dims, floor_at_min_value):
    """Inside the source (0 <= t64 <= s - 1 by 1e-3 on every axis) n-linear interpolation
    of the linear f is exact, so
        |got - max(1e-4, f(t64))| <= 16 * 2^-24 * max|f| + sum_d |slope_d| * ulp32(max|t_d|)
    (8 float roundings + 7 float adds of the accumulation; the float32 position);
    outside [0, s) by the same margin the result is exactly 0.  t64 comes from
    numpy.linalg.inv, not from the oracle's cofactor inverse."""
    f, inside, outside, t = rc.ramp_reference(m, bb_min, bb_dims)
    want = np.maximum(1e-4, f) if floor_at_min_value else f
    bound = rc.ramp_bound(t[inside])
    err = np.abs(got.astype(np.float64) - want)[inside]
    print("ramp max error", err.max(), "bound", bound)
    assert err.max() <= bound
    assert np.array_equal(got[outside], np.zeros(int(outside.sum()), np.float32))


@pytest.mark.parametrize("name", sorted(rc.ramp_models()))
def test_analytic_ramp_prepare_inputs(gpu, name):
    m, b0, bd = rc.ramp_models()[name]
    imgs, _, _ = prepare_inputs([rc.ramp_source()], [m], b0, bd, weight_type=WeightType.NO_WEIGHTS)
    assert_ramp(imgs[0], m, b0, bd, True)


@pytest.mark.parametrize("name", sorted(rc.ramp_models()))
def test_analytic_ramp_fusion(gpu, name):
    m, b0, bd = rc.ramp_models()[name]
    got = fuse_weighted_average([rc.ramp_source()], [m], b0, bd, 1.0, 1, False)
    assert_ramp(got, m, b0, bd, False)


def test_large_coordinates_match_oracle(gpu):
    """Translation and bb_min in the thousands: float(x) + float(bx) and the double ->
    float position at realistic world coordinates."""
    m, b0, bd = rc.ramp_models()["large"]
    src = rc.random_source(rc.RAMP_DIMS, 51)
    imgs, ws, _ = prepare_inputs([src], [m], b0, bd, rc.BORDER, rc.RANGE, WeightType.VIRTUAL_WEIGHTS)
    ei, ew, _ = ir.prepare_inputs([src], [m], b0, bd, rc.BORDER, rc.RANGE, ir.VIRTUAL_WEIGHTS)
    assert_mismatches_on_ties(imgs[0], ei[0], [m], b0, bd)
    assert_weights_close(ws[0], ew[0])
    assert (ei[0] > 0).mean() > 0.3 and ((ew[0] > 0) & (ew[0] < 1)).any()
    ds, ds_dims = rc.LARGE_DS, rc.large_ds_dims(bd)
    for interp in (1, 0):
        got = fuse_weighted_average([src], [m], b0, ds_dims, ds, interp, True, [(1, 0, 1)], [(5, 6, 4)])
        want = fr.fuse_weighted_average([src], [m], b0, ds_dims, ds, interp, True, [(1, 0, 1)], [(5, 6, 4)])
        assert_mismatches_on_ties(got, want, [m], b0, ds_dims, ds, half=(interp == 0))
        assert (want > 0).mean() > 0.3


# ---------------------------------------------------------------- 6. view counts
@pytest.mark.parametrize("wt", list(WeightType))
@pytest.mark.parametrize("V", [1, 7])
def test_view_counts_prepare_inputs(gpu, V, wt):
    srcs, models, b0, bd = rc.count_case(V)
    imgs, ws, info = prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, wt)
    ei, ew, _ = ir.prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, int(wt))
    for v in range(V):
        assert_mismatches_on_ties(imgs[v], ei[v], [models[v]], b0, bd)
        assert_weights_close(ws[v], ew[v])
    if wt != WeightType.NO_WEIGHTS:
        _, _, mn, av = ir.normalize_weights(list(rc.raw_weights(f"count{V}", int(wt))), int(wt), 8)
        assert_overlap_stats(info, mn, av, 8)
    if wt == WeightType.PRECOMPUTED_WEIGHTS:
        # NaN exactly where no view has a weight; elsewhere each w_v / sum is rounded to
        # float once (relative 2^-24), so the V weights sum to 1 within V * 2^-24
        rawsum = sum(w.astype(np.float64) for w in rc.raw_weights(f"count{V}", ir.PRECOMPUTED_WEIGHTS))
        for v in range(V):
            np.testing.assert_array_equal(np.isnan(ws[v]), rawsum == 0)
        total = sum(w.astype(np.float64) for w in ws)
        assert (rawsum > 0).any() and (rawsum == 0).any()
        assert np.abs(total[rawsum > 0] - 1.0).max() <= V * 2.0 ** -24


@pytest.mark.parametrize("interp,blend", [(1, True), (0, True), (1, False)])
@pytest.mark.parametrize("V", [1, 7])
def test_view_counts_fusion(gpu, V, interp, blend):
    srcs, models, b0, bd = rc.count_case(V)
    b, r = rc.COUNT_FUSE_BORDERS[:V], rc.COUNT_FUSE_RANGES[:V]
    got = fuse_weighted_average(srcs, models, b0, bd, 1.0, interp, blend, b, r)
    want = fr.fuse_weighted_average(srcs, models, b0, bd, 1.0, interp, blend, b, r)
    assert_mismatches_on_ties(got, want, models, b0, bd, half=(interp == 0))
    assert (want > 0).any() and (want == 0).any()


# ---------------------------------------------------------------- 7. device-resident paths
@pytest.mark.parametrize("wt", list(WeightType))
def test_prepare_inputs_device_equals_host(gpu, wt):
    srcs, models, b0, bd = rc.base_case()
    hi, hw, hinfo = prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, wt, 2, 1.0)
    dsrcs = [torch.from_numpy(s).cuda() for s in srcs]
    di, dw, dinfo = prepare_inputs(dsrcs, models, b0, bd, rc.BORDER, rc.RANGE, wt, 2, 1.0)
    torch.cuda.synchronize()
    for v in range(len(srcs)):
        assert di[v].is_cuda and dw[v].is_cuda
        np.testing.assert_array_equal(di[v].cpu().numpy(), hi[v])
        np.testing.assert_array_equal(dw[v].cpu().numpy(), hw[v])   # NaN == NaN here
        assert (hi[v] > 0).any()
    for k in ("osem", "min_overlap", "avg_overlap"):
        np.testing.assert_array_equal(dinfo[k], hinfo[k])


@pytest.mark.parametrize("sigmas", [None, ((2, 2, 2), (4, 4, 4))], ids=["plain", "content"])
def test_fusion_device_equals_host(gpu, sigmas):
    """src_on_device / out_on_device of spim_fusion_params, which the Python wrapper
    never sets: the same kernels on the caller's device buffers."""
    srcs, models, b0, bd = rc.base_case(2)
    b, r = rc.BASE_FUSE_BORDERS, rc.BASE_FUSE_RANGES
    sh, host = fuse_raw(srcs, models, b0, bd, 1.0, 1, True, b, r, sigmas)
    sd, dev = fuse_raw(srcs, models, b0, bd, 1.0, 1, True, b, r, sigmas, on_device=True)
    assert sh == 0 and sd == 0, _lib.last_error()
    np.testing.assert_array_equal(dev, host)
    assert (host > 0).any() and (host == 0).any()
    if sigmas is None:
        want = fr.fuse_weighted_average(srcs, models, b0, bd, 1.0, 1, True, b, r)
        assert_mismatches_on_ties(host, want, models, b0, bd)
    else:
        wrapped = fuse_weighted_average(srcs, models, b0, bd, 1.0, 1, True, b, r, use_content_based=True,
                                        content_sigma1=sigmas[0], content_sigma2=sigmas[1])
        np.testing.assert_array_equal(host, wrapped)


# ---------------------------------------------------------------- 8. argument errors
def _bad_prepare(**kw):
    srcs, models, b0, bd = rc.base_case()
    args = dict(srcs=srcs, models=models, bb_min=b0, bb_dims=bd, blending_border=rc.BORDER,
                blending_range=rc.RANGE, weight_type=WeightType.VIRTUAL_WEIGHTS)
    args.update(kw)
    with pytest.raises(_lib.SpimDeconError) as e:
        prepare_inputs(**args)
    return e.value.status


def test_argument_errors_leave_the_library_usable(gpu):
    """Host-side argument checks: SPIMDECON_ERR_ARG, no kernel launched, and the next
    valid call gives the result it gave before."""
    srcs, models, b0, bd = rc.base_case()
    good = lambda: prepare_inputs(srcs, models, b0, bd, rc.BORDER, rc.RANGE, WeightType.VIRTUAL_WEIGHTS, 2, 1.0)
    i0, w0, info0 = good()
    singular = [models[0], np.hstack([np.outer([1.0, 2.0, 3.0], [1.0, 0.5, 0.25]), np.zeros((3, 1))]), models[2]]
    assert _bad_prepare(models=singular) == SPIMDECON_ERR_ARG
    assert "invertible" in _lib.last_error()
    assert _bad_prepare(ij_threads=0) == SPIMDECON_ERR_ARG
    assert _bad_prepare(weight_type=7) == SPIMDECON_ERR_ARG
    for dims in ((0, 34, 30), (40, 0, 30), (40, 34, 0)):
        assert _bad_prepare(bb_dims=dims) == SPIMDECON_ERR_ARG
    i1, w1, info1 = good()
    for v in range(len(srcs)):
        np.testing.assert_array_equal(i1[v], i0[v])
        np.testing.assert_array_equal(w1[v], w0[v])
    assert info1 == info0

    b, r = rc.BASE_FUSE_BORDERS, rc.BASE_FUSE_RANGES
    s0, f0 = fuse_raw(srcs[:2], models[:2], b0, bd, 1.0, 1, True, b, r)
    assert s0 == 0
    assert fuse_raw(srcs[:2], models[:2], b0, bd, 1.0, 2, True, b, r)[0] == SPIMDECON_ERR_ARG
    assert fuse_raw(srcs[:2], models[:2], b0, bd, 1.0, 1, True, None, None)[0] == SPIMDECON_ERR_ARG
    assert fuse_raw(srcs[:2], models[:2], b0, bd, 1.0, 1, True, b, None)[0] == SPIMDECON_ERR_ARG
    assert fuse_raw(srcs[:2], singular[:2], b0, bd, 1.0, 1, True, b, r)[0] == SPIMDECON_ERR_ARG
    assert fuse_raw(srcs[:2], models[:2], b0, (40, 34, 0), 1.0, 1, True, b, r)[0] == SPIMDECON_ERR_ARG
    s1, f1 = fuse_raw(srcs[:2], models[:2], b0, bd, 1.0, 1, True, b, r)
    assert s1 == 0
    np.testing.assert_array_equal(f1, f0)
    np.testing.assert_array_equal(f0, fuse_weighted_average(srcs[:2], models[:2], b0, bd, 1.0, 1, True, b, r))
