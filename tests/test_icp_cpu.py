"""CPU: the ICP restatement (tests/icp_ref.py) -- its literal ambiguity removal against the
claim-count form, the scenario of the reference's own ``main``, convergence and limits, a planted
rigid motion recovered -- driven through ``registration.icp`` with ``assign=icp_ref.assign``,
the premises of the GPU cases (tests/test_gpu_icp.py), and the C-ABI's host-side rules."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import icp_ref as ir
from spim_registration_amd import _lib, globalopt, registration

F32, F64 = np.float32, np.float64


def run_icp(pa, pb, model, **kw):
    """registration.icp over the restatement's assignment, checked against the restatement's loop"""
    got = registration.icp(pa, pb, model, assign=ir.assign, **kw)
    want = ir.icp(pa, pb, model, **kw)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    if want[2] is None:
        assert got[2] is None and np.isnan(got[3]) and np.isnan(want[3])
    else:
        np.testing.assert_array_equal(got[2], want[2])
        assert got[3] == want[3]
    assert got[4] == want[4]
    return got


# ---------------------------------------------------------------- removeAmbigousMatches
def check_ambiguous(it, ir_):
    left, removed = ir.remove_ambiguous_literal(list(zip(it, ir_)))
    kt, kr, n = ir.remove_ambiguous(it, ir_)
    assert left == list(zip(kt.tolist(), kr.tolist())) and n == len(removed)
    assert sorted(left + removed) == sorted(zip(it, ir_))
    return len(left), n


@pytest.mark.parametrize("n", [0, 1, 2, 60])
def test_literal_removal_equals_claim_counts(n):
    """random match lists, every reference point once, the targets drawn from few values so that
    most are claimed twice or more"""
    rng = np.random.default_rng(30 + n)
    ambiguous = 0
    for _ in range(20):
        it = rng.integers(0, max(n // 3, 2), n).tolist()
        ir_ = np.sort(rng.permutation(4 * n + 1)[:n]).tolist()
        ambiguous += check_ambiguous(it, ir_)[1]
    assert ambiguous > 0 or n < 2


def test_literal_removal_without_and_with_only_ambiguity():
    assert check_ambiguous([5, 3, 9, 0], [0, 1, 2, 7]) == (4, 0)
    assert check_ambiguous([4, 4, 2, 2, 2], [0, 3, 4, 8, 9]) == (0, 5)
    assert check_ambiguous([4, 1, 4], [0, 1, 2]) == (1, 2)


# ---------------------------------------------------------------- the reference's main
def test_the_scenario_of_the_reference_main():
    """IterativeClosestPointPairwise.java:138-213 (its random coordinates replaced by fixed ones
    at least 150 apart): one pair off by (1, 3, 0), d = 3.16, five off by (2, 4, 0), d = 4.47 > 4.
    Iteration 0 matches the first, translation (1, 3, 0); under it the five are 1.41 away:
    iteration 1 has all 6, translation the mean (11/6, 23/6, 0); iteration 2 repeats it"""
    a = np.array([[10.0, 10, 0]] + [[150.0 + 1000 * k, 300.0 + 700 * k, 0] for k in range(1, 6)])
    b = a + np.array([[1.0, 3, 0]] + [[2.0, 4, 0]] * 5)
    counts = []

    def spy(*args, **kw):
        out = ir.assign(*args, **kw)
        counts.append(len(out[0]))
        return out
    it, ir_, m, err, i = registration.icp(a, b, "translation", max_distance=4.0, assign=spy)
    assert counts == [1, 6, 6] and i == 2
    np.testing.assert_array_equal(it, np.arange(6))
    np.testing.assert_array_equal(ir_, np.arange(6))
    assert np.abs(m[:, 3] - [11 / 6, 23 / 6, 0]).max() < 1e-12 and np.array_equal(m[:, :3], np.eye(3))
    assert abs(err - (np.hypot(5 / 6, 5 / 6) + 5 * np.hypot(1 / 6, 1 / 6)) / 6) < 1e-12
    run_icp(a, b, "translation", max_distance=4.0)


# ---------------------------------------------------------------- convergence and limits
def test_max_iterations_bounds_the_loop():
    """3 degrees and (3, -2, 1): the first assignment reaches a fraction of the pairs, every fit
    brings more within 5 px"""
    a, b = ir.recovery_case(motion=ir.FAR_MOTION)
    full = run_icp(a, b, "rigid")
    assert 3 <= full[4] < 100 and np.abs(full[2] - ir.FAR_MOTION).max() < 0.1
    two = run_icp(a, b, "rigid", max_iterations=2)
    assert two[4] == 2
    one = run_icp(a, b, "rigid", max_iterations=1)
    assert one[4] == 1 and len(one[0]) < len(two[0]) // 2
    want = ir.assign(a, b)                                     # the identity's assignment, fitted once
    np.testing.assert_array_equal(one[0], want[0])
    np.testing.assert_array_equal(one[2], globalopt.fit("rigid", a[want[0]], b[want[1]], np.ones(len(want[0]))))


@pytest.mark.parametrize("model,na,nb", [("affine", 3, 50), ("affine", 50, 3), ("rigid", 2, 2), ("translation", 0, 5)])
def test_lists_below_the_minimum(model, na, nb):
    a, b = ir.recovery_case()
    it, ir_, m, err, i = run_icp(a[:na], b[:nb], model)
    assert len(it) == len(ir_) == 0 and m is None and np.isnan(err) and i == 0


def test_no_match_inside_max_distance():
    a, b = ir.recovery_case()
    it, ir_, m, err, i = run_icp(a, b + 1000.0, "translation")
    assert len(it) == len(ir_) == 0 and m is None and np.isnan(err) and i == 0


def test_ill_defined_matches_are_a_failure():
    """five coplanar matches: the affine fit is singular"""
    a = np.array([[0.0, 0, 0], [50, 0, 0], [0, 50, 0], [50, 50, 0], [100, 20, 0]])
    it, _, m, err, i = run_icp(a, a + 0.5, "affine")
    assert len(it) == 0 and m is None and np.isnan(err) and i == 0


# ---------------------------------------------------------------- recovery
def test_recovers_a_planted_rigid_motion():
    a, b = ir.recovery_case()
    _, _, nearest, dist, ambiguous = ir.assign(a, b, return_all=True)
    assert ambiguous > 0 and (dist > 5.0).sum() > 0            # the first iteration has both
    it, ir_, m, err, i = run_icp(a, b, "rigid")
    assert len(it) > 120 and err < 0.3
    assert np.abs(m[:, 3] - ir.RECOVERY_MOTION[:, 3]).max() < 0.05
    assert np.abs(m[:, :3] - ir.RECOVERY_MOTION[:, :3]).max() < 1e-3


def test_pairwise_and_register_icp_on_the_restatement():
    pts, true, given = ir.registration_scene()
    matches = registration.pairwise_icp(pts, given, model="rigid", assign=ir.assign)
    assert len(matches) == 6 and all(len(m.pa) == len(m.pb) > 200 for m in matches)
    got, res = registration.register_icp(pts, given, model="rigid", assign=ir.assign)
    assert res is not None and not res.unaligned and res.failure is None
    for g, t, g0 in zip(got[1:], true[1:], given[1:]):
        assert np.linalg.norm(g0[:, 3] - t[:, 3]) > 1.0
        assert np.abs(g[:, 3] - t[:, 3]).max() < 1e-2
    with pytest.raises(ValueError):
        registration.icp(pts[0], pts[1], "bogus", assign=ir.assign)


# ---------------------------------------------------------------- premises of the GPU cases
@pytest.mark.parametrize("model", [None, ir.AFFINE], ids=["identity", "affine"])
def test_size_cases_hold_matches_non_matches_and_ambiguous_claims(model):
    for seed, nt, nr in ir.SIZE_CASES + [ir.SPLIT_CASE]:
        t, r = ir.make_case(seed, nt, nr, model)
        it, ir_, nearest, dist, ambiguous = ir.assign(t, r, model, return_all=True)
        assert np.isfinite(dist).all() and nearest.min() >= 0 and nearest.max() < nt
        if min(nt, nr) >= 100:
            assert len(it) > nr // 10 and ambiguous >= 2 and (dist > 5.0).sum() > nr // 10
            assert len(it) + ambiguous + (dist > 5.0).sum() == nr
    t, r = ir.make_case(902, 1, 300)
    assert ir.assign(t, r, return_all=True)[4] > 100           # one target, claimed by many


def test_equal_float_case_holds_different_doubles():
    t, r = ir.equal_float_case()
    s = ir.distance_sums(t[None, :, :], r[:, None, :])
    d = ir.distances(t, r)
    _, _, nearest, dist, _ = ir.assign(t, r, return_all=True)
    k = np.arange(len(r))
    np.testing.assert_array_equal(nearest, 2 * k)              # the lower index of each pair
    assert np.all(d[k, 2 * k] == d[k, 2 * k + 1]) and np.all(dist == F32(5.0))
    assert np.all(s[k, 2 * k] != s[k, 2 * k + 1])
    assert (s[k, 2 * k] > s[k, 2 * k + 1]).sum() == len(r) // 2   # ... although it is the farther one


def test_lattice_case_holds_eight_way_ties():
    t, r = ir.lattice_case()
    d = ir.distances(t, r)
    assert np.all((d == d.min(axis=1, keepdims=True)).sum(axis=1) == 8)
    it, ir_, nearest, _, ambiguous = ir.assign(t, r, return_all=True)
    corner = np.floor(r).astype(int)
    np.testing.assert_array_equal(nearest, (corner[:, 0] * 4 + corner[:, 1]) * 4 + corner[:, 2])
    assert ambiguous == 0 and len(it) == 27


def test_ambiguity_case_is_what_it_says():
    t, r, (it, ir_), ambiguous = ir.ambiguity_case()
    got = ir.assign(t, r, return_all=True)
    np.testing.assert_array_equal(got[0], it)
    np.testing.assert_array_equal(got[1], ir_)
    assert got[4] == ambiguous and got[3][2] == F32(7.0) and got[2][2] == 2


def test_fma_cases_round_differently_when_fused():
    """the x row evaluated exactly with one rounding after m0 x + y (a fused multiply-add) casts
    to another float than the separately rounded chain of the restatement"""
    for model, t, r in ir.fma_cases():
        x, y = t[0, 0], t[0, 1]
        fused = float(Fraction(model[0, 0]) * Fraction(x) + Fraction(y))     # one correctly rounded result
        w = ir.apply(model, t)
        assert w[0, 1] == 0.0 and w[0, 2] == 0.0
        assert F32(fused) != F32(w[0, 0]) and abs(fused - w[0, 0]) < 1e-10
        _, _, _, dist, _ = ir.assign(t, r, model, return_all=True)
        assert dist[0] == F32(w[0, 0])


def test_apply_and_distance_are_the_stated_chains():
    rng = np.random.default_rng(41)
    p = rng.uniform(-300, 300, (50, 3))
    w = ir.apply(ir.AFFINE, p)
    for k in (0, 17, 49):
        x, y, z = (F64(v) for v in p[k])
        for row in range(3):
            m = [F64(v) for v in ir.AFFINE[row]]
            assert w[k, row] == ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
    assert np.abs(w - globalopt.apply(ir.AFFINE, p)).max() < 1e-10
    np.testing.assert_array_equal(ir.apply(None, p), p)
    o = rng.uniform(-300, 300, 3)
    for k in (0, 17):
        dx, dy, dz = (F64(F32(o[c]) - F32(p[k, c])) for c in range(3))
        assert ir.distance_to(p[k], o) == F32(np.sqrt(dx * dx + dy * dy + dz * dz))


# ---------------------------------------------------------------- the C ABI's host side
def test_defaults_and_tiles(lib):
    p = _lib.IcpParams()
    lib.spim_icp_params_default(C.byref(p))
    assert (p.max_distance, p.max_iterations, p.t_split, p.device) == (5.0, 100, 0, 0)
    assert C.sizeof(_lib.IcpParams) == 16
    assert registration.icp_tile_sizes() == (ir.R_BLOCK, ir.T_TILE)


def test_argument_rules_need_no_gpu(lib):
    p = _lib.IcpParams()
    lib.spim_icp_params_default(C.byref(p))
    pts = np.zeros((4, 3))
    nearest, dist = np.zeros(4, np.int32), np.zeros(4, np.float32)
    mt, mr = np.zeros(4, np.int32), np.zeros(4, np.int32)
    n, amb = C.c_int64(-1), C.c_int64(-1)

    def run(nt=4, nr=4, params=p, count=n):
        return lib.spim_icp_assign(pts.ctypes.data, nt, pts.ctypes.data, nr, None,
                                   C.byref(params) if params is not None else None, nearest.ctypes.data,
                                   dist.ctypes.data, mt.ctypes.data, mr.ctypes.data, 4,
                                   C.byref(count) if count is not None else None, C.byref(amb))
    assert run(params=None) == -1
    assert run(count=None) == -1
    assert run(nt=2 ** 31) == -1 and "2^31" in _lib.last_error()
    assert run(nr=-1) == -1
    q = _lib.IcpParams()
    lib.spim_icp_params_default(C.byref(q))
    q.t_split = -1
    assert run(params=q) == -1 and "t_split" in _lib.last_error()
