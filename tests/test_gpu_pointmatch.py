"""The three point-list matchers (csrc/rgldm.hip, geohash.hip, icp.hip) share one host scaffold
(csrc/pointmatch.hpp) over persistent, grow-only workspaces: a call must not depend on what ran
before it.  One process, one device, one fixed order of calls -- growing, shrinking (stale tails
in every buffer), the below-minimum and empty paths, a capacity failure and the call after it --
each equal to its restatement (tests/rgldm_ref.py, gh_ref.py, icp_ref.py) bit for bit, compared
as tests/test_gpu_{rgldm,gh,icp}.py compare."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import gh_ref as gr
import icp_ref as ir
import rgldm_ref as rr
from spim_registration_amd import _lib, registration

pytestmark = pytest.mark.gpu

# (seed, na, nb): 300 x 333 straddles RGLDM's A tile (128) and B tile (64) and geometric
# hashing's 256 / 256; 130 x 65 is smaller in both lists.  (seed, nt, nr): 1030 x 260 straddles
# ICP's target tile (1024) and reference block (256).
RG_LARGE, RG_SMALL = (1201, 300, 333), (1204, 130, 65)
GH_SMALL, GH_LARGE = (1202, 130, 65), (1205, 300, 333)
ICP_CASE = (1203, 1030, 260)


@functools.lru_cache(maxsize=None)
def rg_case(case):
    a, b = rr.make_pair(*case)
    return a, b, rr.rgldm(a, b)


@functools.lru_cache(maxsize=None)
def gh_case(case):
    a, b = gr.make_pair(*case)
    return a, b, gr.geometric_hashing(a, b)


@functools.lru_cache(maxsize=None)
def icp_case():
    t, r = ir.make_case(*ICP_CASE, ir.AFFINE)
    return t, r, ir.assign(t, r, ir.AFFINE, return_all=True)


def same_bits(got, want, nan_equal=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    g, w = got.view(np.uint64), want.view(np.uint64)
    if nan_equal:   # (tests/test_gpu_gh.py: two NaNs are equal whatever their payload)
        nan = np.isnan(got) & np.isnan(want)
        g, w = np.where(nan, 0, g), np.where(nan, 0, w)
    np.testing.assert_array_equal(g, w)


def check_candidates(fn, a, b, want, nan_equal):
    ia, ib, idx, best, second = fn(a, b, return_all=True)
    np.testing.assert_array_equal(idx, want["best_idx"])
    same_bits(best, want["best"], nan_equal)
    same_bits(second, want["second"], nan_equal)
    assert ia.dtype == ib.dtype == np.int32
    np.testing.assert_array_equal(ia, want["ia"])
    np.testing.assert_array_equal(ib, want["ib"])
    return ia


def check_rgldm(a, b, want):
    return check_candidates(registration.rgldm_candidates, a, b, want, False)


def check_gh(a, b, want):
    return check_candidates(registration.gh_candidates, a, b, want, True)


def check_icp(t, r, want, model):
    it, ir_, nearest, dist, ambiguous = registration.icp_assign(t, r, model, return_all=True)
    assert it.dtype == ir_.dtype == nearest.dtype == np.int32 and dist.dtype == np.float32
    np.testing.assert_array_equal(nearest, want[2])
    np.testing.assert_array_equal(dist.view(np.uint32), want[3].view(np.uint32))
    np.testing.assert_array_equal(it, want[0])
    np.testing.assert_array_equal(ir_, want[1])
    assert ambiguous == want[4]
    return it


def check_below_minimum(check, ref, a, b):
    """the fill values for every A point, no candidate"""
    want = ref(a, b)
    assert np.all(want["best"] == rr.DOUBLE_MAX) and np.all(want["second"] == rr.DOUBLE_MAX)
    assert np.all(want["best_idx"] == -1) and len(want["best"]) == len(a) and len(want["ia"]) == 0
    assert len(check(a, b, want)) == 0


def test_calls_do_not_depend_on_the_calls_before(gpu, lib):
    # 1: grows RGLDM's buffers
    a1, b1, want1 = rg_case(RG_LARGE)
    assert len(check_rgldm(a1, b1, want1)) > 0
    # 2
    assert len(check_gh(*gh_case(GH_SMALL))) > 0
    # 3
    assert len(check_icp(*icp_case(), ir.AFFINE)) > 0
    # 4: smaller than call 1, stale tails in every buffer
    assert len(check_rgldm(*rg_case(RG_SMALL))) > 0
    # 5: larger than call 2
    a5, b5, want5 = gh_case(GH_LARGE)
    assert len(check_gh(a5, b5, want5)) > 0
    # 6: nb = 3, below both minima, over buffers that hold the results above
    check_below_minimum(check_rgldm, rr.rgldm, a1, b1[:3])
    check_below_minimum(check_gh, gr.geometric_hashing, a5, b5[:3])
    # 7: no target
    _, r, _ = icp_case()
    none = np.zeros((0, 3))
    want = ir.assign(none, r, ir.AFFINE, return_all=True)
    assert np.all(want[2] == -1) and np.all(want[3] == ir.FLOAT_MAX) and len(want[2]) == len(r)
    assert len(check_icp(none, r, want, ir.AFFINE)) == 0
    # 8: a capacity failure, then the same call with room
    na, nb = len(a1), len(b1)
    a, b = np.ascontiguousarray(a1), np.ascontiguousarray(b1)
    need = len(want1["ia"])
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
    assert run(need - 1) == -1 and "capacity" in _lib.last_error()
    assert run(na) == 0 and n.value == need
    np.testing.assert_array_equal(idx, want1["best_idx"])
    same_bits(best, want1["best"])
    same_bits(second, want1["second"])
    np.testing.assert_array_equal(ia[:need], want1["ia"])
    np.testing.assert_array_equal(ib[:need], want1["ib"])
    assert np.all(ia[need:] == -7)
    check_rgldm(a1, b1, want1)
