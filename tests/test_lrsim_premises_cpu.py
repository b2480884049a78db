"""The cases of tests/lrsim_cases.py hit what they are named for -- proved on the launch
arithmetic of csrc/lrsim.hip (restated in lrsim_cases.py) and on the oracle, no GPU."""
import numpy as np
import pytest

import lrsim_cases as lc
from oracle import lrsim_ref as ref


def test_fft_fast_size_restatement():
    """Known values of csrc/fft.cpp's fft_fast_size: 2,3,5,7-smooth, even on request."""
    assert [lc.fft_fast_size(n, False) for n in (0, 1, 5, 9, 11, 13, 23, 26, 132, 422)] == \
        [1, 1, 5, 9, 12, 14, 24, 27, 135, 432]
    assert [lc.fft_fast_size(n, True) for n in (1, 5, 9, 12, 13, 27, 52, 422)] == [2, 6, 10, 12, 14, 28, 54, 432]
    assert lc.padded((3, 7, 10), [lc.K3]) == (5, 9, 12) and lc.ncplx((3, 7, 10), [lc.K3]) == 315


@pytest.mark.parametrize("shape,ksizes", lc.EXISTING)
def test_existing_shapes_never_ran_the_odd_tail(shape, ksizes):
    """Every volume of tests/test_gpu_lrsim.py has an even ncplx (k_lr_cmul's and
    k_spec_mul's single-value tail is dead there), makes one trip through every grid-stride
    loop and leaves fewer block partials than one sweep of the reductions."""
    assert lc.ncplx(shape, ksizes) % 2 == 0
    n = int(np.prod(shape))
    mz, my, _ = lc.padded(shape, ksizes)
    assert lc.voxel_trips(n) == 1 and lc.row_trips(my * mz) == 1 and lc.row_trips(shape[0] * shape[1]) == 1
    assert lc.blocks(n, lc.BLOCK) < lc.REDUCE_THREADS
    assert lc.EXISTING[0][0] == (40, 36, 44) and lc.padded(*lc.EXISTING[0]) == (50, 45, 54)


def test_odd_tail_cases():
    for name in ("odd_tail", "odd_tail_slack"):
        c = lc.CASES[name]
        mz, my, mx = lc.padded(c.shape, c.ksizes)
        assert (mx // 2 + 1) % 2 == 1 and my % 2 == 1 and mz % 2 == 1
        assert lc.ncplx(c.shape, c.ksizes) % 2 == 1
    assert lc.padded(lc.CASES["odd_tail"].shape, lc.CASES["odd_tail"].ksizes) == (5, 9, 12)
    # slack (M > n + 2 c) with an odd tail, and odd My, Mz under an even Hx with slack in x
    c = lc.CASES["odd_tail_slack"]
    assert lc.padded(c.shape, c.ksizes)[0] == 27 > c.shape[0] + 2
    c = lc.CASES["odd_tail_even_hx"]
    mz, my, mx = lc.padded(c.shape, c.ksizes)
    assert (mx // 2 + 1) % 2 == 0 and my % 2 == 1 and mz % 2 == 1 and mx > c.shape[2] + 2


def test_odd_dims_case():
    c = lc.CASES["odd_dims"]
    assert all(s % 2 == 1 and s % 64 != 0 for s in c.shape) and len(c.ksizes) == 3
    for d in range(3):
        assert len({k[d] for k in c.ksizes}) == 3            # three kernel sizes on every axis
    for k in c.ksizes:
        assert len(set(k)) == 3                              # and three sizes per kernel
    _, ws, _ = lc.build("odd_dims")
    assert (lc.positive_count(ws) == 0).any()                # some voxels end at minValue


def test_many_voxels_takes_a_second_trip():
    c = lc.CASES["many_voxels"]
    n = int(np.prod(c.shape))
    assert lc.VOXELS_PER_SWEEP < n < 1.02 * lc.VOXELS_PER_SWEEP and lc.voxel_trips(n) == 2
    assert lc.blocks(n, lc.BLOCK) == lc.MAX_BLOCKS > lc.REDUCE_THREADS   # the reductions loop too
    assert c.iters == 1 and set(c.rules) == {(False, 0.0), (True, 0.0), (False, 0.006), (True, 0.006)}
    # the voxels of the second trip are not all alike: they carry zero and positive weights
    _, ws, _ = lc.build("many_voxels")
    tail = lc.positive_count(ws).reshape(-1)[lc.VOXELS_PER_SWEEP:]
    assert (tail == 0).any() and (tail == 2).any()
    # and the block partials beyond the first 1024 matter for the initial average
    assert (lc.nonzero_count(ws).reshape(-1)[lc.REDUCE_THREADS * lc.BLOCK:] > 1).any()


def test_many_rows_takes_a_second_trip():
    c = lc.CASES["many_rows"]
    mz, my, _ = lc.padded(c.shape, c.ksizes)
    assert c.shape[0] * c.shape[1] > lc.ROWS_PER_SWEEP and lc.row_trips(c.shape[0] * c.shape[1]) == 2
    assert my * mz > lc.ROWS_PER_SWEEP and lc.row_trips(my * mz) == 2
    assert c.shape[2] < 64 and int(np.prod(c.shape)) < lc.VOXELS_PER_SWEEP


@pytest.mark.parametrize("name", sorted(lc.LONG_REACH))
def test_long_reach_folds_twice(name):
    c = lc.CASES[name]
    d = lc.LONG_REACH[name]
    n, r = c.shape[d], lc.reach(c.ksizes)[d]
    assert n in (2, 3) and max(k[d] for k in c.ksizes) in (7, 9)
    assert r >= n and lc.mirror_folds(r, n) >= 2
    for o in range(3):
        if o != d:
            assert lc.reach(c.ksizes)[o] < c.shape[o]
    # the oracle's extension folds the same way: numpy's 'reflect' has period 2 (n - 1)
    a = np.arange(n, dtype=np.float32)
    ext = np.pad(a, (r, r), mode="reflect")
    p = 2 * (n - 1)
    want = [min(j % p, p - j % p) for j in range(-r, n + r)]
    assert ext.tolist() == want
    assert {k for k in lc.LONG_REACH if k.endswith("2")} and {lc.LONG_REACH[k] for k in lc.LONG_REACH} == {0, 1, 2}


def test_weights_regions():
    imgs, ws, _ = lc.build("weights")
    pos, nz = lc.positive_count(ws), lc.nonzero_count(ws)
    for v, w in enumerate(ws):
        assert (w == 0).any() and (w < 0).any() and (w > 0).any(), v       # per view: zeros, negatives
    assert (nz[lc.rows("zero")] == 0).all() and (pos[lc.rows("zero")] == 0).all()
    assert (nz[lc.rows("negative")] == 3).all() and (pos[lc.rows("negative")] == 0).all()
    assert (nz[lc.rows("single")] == 1).all() and (pos[lc.rows("single")] == 1).all()
    assert (nz[lc.rows("mixed")] == 2).all() and (pos[lc.rows("mixed")] == 1).all()
    assert (pos[lc.rows("all")] == 3).all()
    for r in lc.REGION_ROWS:
        assert pos[lc.rows(r)].size > 0
    assert (pos != nz).any()             # the != 0 overlap count and the > 0 num disagree
    # swapping either condition changes the oracle: the average over > 0 instead of != 0 ...
    avg = ref.norm_all_images(imgs, ws)
    assert abs(ref.norm_all_images(imgs, [np.where(w > 0, w, 0) for w in ws]) - avg) > 1e-6 * avg
    # ... and num over != 0 instead of > 0 on the mixed rows (where the result is not clamped)
    num_pos = sum(np.where(w > 0, w, 0).astype(np.float64) for w in ws)
    num_nz = sum(w.astype(np.float64) for w in ws)
    assert (np.abs(num_pos - num_nz)[lc.rows("mixed")] > 0.05).all()
    # the oracle ends at minValue exactly where no view is positive
    for mult, lam in lc.CASES["weights"].rules:
        psi, _, _ = lc.oracle("weights", mult, lam)
        assert np.array_equal(psi == lc.MIN32, pos == 0), (mult, lam)


def test_no_overlap_average_is_one():
    imgs, ws, _ = lc.build("no_overlap")
    nz = lc.nonzero_count(ws)
    assert nz.max() == 1 and (nz == 0).any() and all((w != 0).any() for w in ws)
    assert ref.norm_all_images(imgs, ws) == 1.0
    assert lc.oracle("no_overlap", False, 0.0)[1] == 1.0


@pytest.mark.parametrize("mult", [False, True])
def test_delta_is_the_weighted_mean(mult):
    """1x1x1 kernels: c = 0, and one iteration is the weighted arithmetic (geometric, when
    multiplicative) mean of the views (as test_identity_kernel_one_iteration_is_weighted_mean)."""
    c = lc.CASES["delta"]
    assert lc.reach(c.ksizes) == (0, 0, 0) and c.iters == 1 and (mult, 0.0) in c.rules
    imgs, ws, _ = lc.build("delta")
    psi, avg, _ = lc.oracle("delta", mult, 0.0)
    np.testing.assert_allclose(psi, lc.delta_closed_form(imgs, ws, avg, mult), rtol=2e-6)


@pytest.mark.parametrize("mult,lam", lc.CASES["clamp"].rules)
def test_clamp_set_does_not_depend_on_rounding_noise(mult, lam):
    """The zero block is wider than twice the reach, so its core sees only zero quotients:
    the contribution there is rounding noise of either sign, or exactly 0, and every one of
    them ends at minValue.  Float64 and float32 convolutions agree on the set."""
    c = lc.CASES["clamp"]
    r = lc.reach(c.ksizes)
    for d, s in enumerate(lc.ZERO_BLOCK):
        assert s.stop - s.start > 2 * r[d]
    imgs, ws, _ = lc.build("clamp")
    assert all((i[lc.ZERO_BLOCK] == 0).all() for i in imgs) and all((w > 0).all() for w in ws)
    p64 = lc.oracle_at_precision("clamp", mult, lam, "f64")
    p32 = lc.oracle_at_precision("clamp", mult, lam, "f32")
    assert np.array_equal(p64, lc.oracle("clamp", mult, lam)[0])      # the restated loop is the oracle's
    s64, s32 = p64 == lc.MIN32, p32 == lc.MIN32
    assert s64.any() and np.array_equal(s64, s32)
    core = np.zeros(c.shape, bool)
    core[3:6, 0:4, 5:8] = True          # the block shrunk by the reach (y = 0 mirrors into the block)
    assert np.array_equal(s64, core)
    # everything else stays far from the clamp: no voxel near minValue whose side noise could pick
    assert p64[~core].min() > 100 * lc.MIN32 and p32[~core].min() > 100 * lc.MIN32


@pytest.mark.parametrize("name", sorted(n for n in lc.CASES if n != "many_voxels"))
def test_float_transforms_resolve_every_case(name):
    """The GPU tests hold float transforms to 1e-4 of the float64 oracle.  That is a fair
    demand only of a case whose dynamic range a float transform resolves: the oracle with
    float32 convolutions stays ten times closer.  (A second iteration of `weights` does not:
    2.0e-4 to 2.5e-4, from quotients img / minValue = 1e4 beside quotients of 1; many_voxels
    is one iteration of two 3x3x3 views on positive images, as many_rows, and is left out
    for its size.)"""
    for mult, lam in lc.CASES[name].rules:
        p32 = lc.oracle_at_precision(name, mult, lam, "f32")
        p64 = lc.oracle(name, mult, lam)[0].astype(np.float64)
        assert np.linalg.norm(p32 - p64) / np.linalg.norm(p64) < 1e-5, (mult, lam)


def test_rule_inputs_cover_the_special_values():
    psi, value, num = lc.rule_inputs(True)
    assert psi.size == lc.RULE_N and lc.voxel_trips(lc.RULE_N) == 2 and lc.RULE_N % lc.BLOCK != 0
    tail = slice(lc.VOXELS_PER_SWEEP, None)
    for v in lc.NUM_SPECIAL:
        assert ((num == v) & (np.signbit(num) == np.signbit(v))).any()
    for v in lc.VALUE_SPECIAL:
        hit = np.isnan(value) if np.isnan(v) else (value == v) & (np.signbit(value) == np.signbit(v))
        assert hit.any() and hit[tail].any()
    for v in lc.PSI_SPECIAL:
        assert (psi == np.float32(v)).any()
    for lam in lc.RULE_LAMBDAS[1:]:      # Tikhonov's radicand goes negative for every lambda
        f = ref.apply_value(psi, value, num, False).astype(np.float64)
        with np.errstate(all="ignore"):
            assert (1.0 + 2.0 * lam * f < 0).any()
    # every class of the result occurs: NaN before the clamp, clamped, kept, infinite
    nxt = ref.apply_value(psi, value, num, False)
    new, s, mx = ref.finish(psi, nxt)
    assert np.isnan(nxt).any() and (new == lc.MIN32).any() and (new > 1).any() and np.isinf(new).any()
    assert np.isinf(s) and np.isinf(mx)
    # the plain inputs keep the statistics finite, so they are compared as numbers
    psi, value, num = lc.rule_inputs(False)
    for mult in (False, True):
        for lam in lc.RULE_LAMBDAS:
            new, s, mx = lc.rule_oracle(psi, value, num, mult, lam)
            assert np.isfinite(s) and np.isfinite(mx) and s > 0, (mult, lam)
