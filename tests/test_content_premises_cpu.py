"""The premises of tests/test_gpu_content_edges.py, proved without a GPU: the fused
multiply-add of tests/content_cases.py is the correctly rounded one, its restatement is
anchored to a float64 sum by a derived bound and to the reference's FFT formulation by the
bound tests/test_gpu_content.py uses, its index rule is extendMirrorSingle's on axes
shorter than the reach, sigma_for_taps gives the tap counts the cases name -- and the
cases can tell the mistakes they are there for (a halo not fetched across a tile seam, a
dropped tap or tap chunk, unfused arithmetic, swapped sigmas, the other mirror rule, an
extremum the reduction misses)."""
import threading
from fractions import Fraction

import numpy as np
import pytest

import content_cases as cc
import content_ref as cr
import test_gpu_content as tgc
from oracle.dog_ref import gaussian_kernel_1d


# ------------------------------------------------------------------ fma32
def _round_to_float32(x: Fraction) -> np.float32:
    """Correct rounding of an exact rational: the nearest of the float32 around it, ties
    to the even mantissa."""
    f = np.float32(float(x))       # within a float32 ulp of x: x lies between f's neighbours
    cand = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    dist = [abs(Fraction(float(c)) - x) for c in cand]
    best = min(dist)
    near = [c for c, d in zip(cand, dist) if d == best]
    if len(near) > 1:
        near = [c for c in near if int(c.view(np.uint32)) & 1 == 0]
    assert len(near) == 1
    return near[0]


def _fma_samples():
    rng = np.random.default_rng(7)
    n = 9000
    # random operands over a wide range of exponents, and sums with heavy cancellation
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    near = rng.random(n) < 0.3
    c[near] = -(a[near].astype(np.float64) * b[near]).astype(np.float32)
    # constructed: a * b = 3 M 2^e with 3 M odd and of 25 bits is exactly the midpoint of two
    # neighbouring float32; c is 0 (a tie: to even) or far below the float64 ulp of the
    # product, so the float64 sum is the midpoint again and only the error term tells on
    # which side the exact value lies
    m = 1500
    M = rng.integers(2 ** 24 // 3 + 1, 2 ** 25 // 3, m) | 1
    assert np.all((3 * M >= 2 ** 24) & (3 * M < 2 ** 25) & (3 * M % 2 == 1) & (M < 2 ** 24))
    e = rng.integers(-30, 30, m)
    a2 = np.float32(3) * np.float32(2.0) ** e.astype(np.float32)
    b2 = M.astype(np.float32)
    assert np.all(b2.astype(np.int64) == M)
    c2 = (rng.choice([-1.0, 0.0, 1.0], m) * 2.0 ** (e - rng.integers(35, 90, m))).astype(np.float32)
    sign = rng.choice([-1.0, 1.0], m).astype(np.float32)
    return (np.concatenate([a, a2 * sign]), np.concatenate([b, b2]), np.concatenate([c, c2 * sign]), n)


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    a, b, c, n_random = _fma_samples()
    assert len(a) >= 10000
    got = cc.fma32(a, b, c)
    assert got.dtype == np.float32 and got.shape == a.shape
    want = np.array([_round_to_float32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], np.float32)
    np.testing.assert_array_equal(got, want)
    # the test discriminates: rounding the float64 sum to float32 rounds twice and is wrong
    # on the constructed samples (and only there, the random ones being far from a midpoint)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    wrong = naive != want
    assert wrong[n_random:].sum() >= 100 and wrong.sum() >= 1
    # and differs from the unfused float32 product and sum in a good part of the random ones
    assert np.mean((a * b + c)[:n_random] != want[:n_random]) > 0.1
    # scalars, broadcasting and non-finite operands
    assert cc.fma32(np.float32(3), np.float32(5), np.float32(0.5)) == np.float32(15.5)
    assert cc.fma32(np.float32([[1], [2]]), np.float32(2), np.float32([1, 2, 3])).shape == (2, 3)
    special = cc.fma32(np.float32([np.inf, np.inf, np.nan, 1.0]), np.float32([2.0, 0.0, 1.0, 1.0]),
                       np.float32([1.0, 1.0, 1.0, -np.inf]))
    assert special[0] == np.inf and np.isnan(special[1]) and np.isnan(special[2]) and special[3] == -np.inf


# ------------------------------------------------------------------ float64 anchor
@pytest.mark.parametrize("K", [3, 49, cc.MAX_TAPS])
def test_ref_pass_within_the_derived_bound_of_float64(K):
    """|ref_pass - the float64 sum| <= gamma_(K + 1) * sum |v k| on every axis; the bound
    is tight enough to notice one dropped tap."""
    img = cc.volume((9, 10, 140), 5)
    sigma = cc.sigma_for_taps(K)
    k = cc.taps(sigma)
    assert len(k) == K
    for axis in range(3):
        out = cc.ref_pass(img, sigma, axis)
        o64, mag = cc.ref_pass64(img, sigma, axis)
        assert out.dtype == np.float32 and o64.dtype == np.float64
        err = np.abs(out.astype(np.float64) - o64)
        assert np.all(err <= cc.pass_bound(K, mag))
        assert err.max() > 0          # (float32 arithmetic: the comparison is not vacuous)
        dropped = k.copy()
        dropped[K // 2 + 1] = 0
        bad = cc.ref_pass(img, sigma, axis, k=dropped)
        assert np.mean(np.abs(bad.astype(np.float64) - o64) > cc.pass_bound(K, mag)) > 0.9


def test_ref_raw64_is_the_chain_of_float64_passes():
    img = cc.volume((5, 6, 7), 6)
    s1, s2 = (1.0, 0.5, 0.8), (1.5, 1.0, 0.4)
    r64, mags = cc.ref_raw64(img, s1, s2)
    assert r64.dtype == np.float64 and len(mags) == 6 and all(m.shape == img.shape for m in mags)
    r32 = cc.ref_raw(img, s1, s2)
    assert r32.dtype == np.float32
    np.testing.assert_allclose(r32, r64, rtol=1e-4)
    assert np.any(r32.astype(np.float64) != r64)


# ------------------------------------------------------------------ the reference's formulation
@pytest.mark.parametrize("name", ["a_multifold_z", "c_one_plane", "d_tile_edges"])
def test_ref_weights_within_the_suites_bound_of_the_fft_restatement(name):
    """The distance of ref_weights from content_ref.content_weights(.., "f64") is within
    the 8 x d32 that test_gpu_content.py allows the GPU; bit equality on the GPU carries
    that over."""
    img, s1, s2, w64, w32 = tgc.case(name)
    got = cc.ref_weights(img, s1, s2)
    assert got.dtype == np.float32 and got.min() == 0.0 and got.max() == 1.0
    d32 = float(np.abs(w32.astype(np.float64) - w64).max())
    dref = float(np.abs(got.astype(np.float64) - w64).max())
    print(f"content restatement {name}: d32 {d32:.3e}  op-order {dref:.3e}  ratio {dref / d32:.2f}")
    assert dref <= 8 * d32, (name, dref, d32)


# ------------------------------------------------------------------ the mirror rule
def _walked_extension(line, reach):
    """``line`` with ``reach`` samples added at each end, built sample by sample by walking
    outwards and turning round at the ends without repeating them."""
    n = len(line)
    sides = []
    for start, step in ((0, -1), (n - 1, 1)):
        pos, dirn, side = start, step, []
        for _ in range(reach):
            if n > 1:
                if not 0 <= pos + dirn < n:
                    dirn = -dirn
                pos += dirn
            side.append(line[pos])
        sides.append(side)
    return np.array(sides[0][::-1] + list(line) + sides[1], np.float32)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_mirror_rule_on_axes_shorter_than_the_reach(n):
    """Reach 231 (463 taps) over 1, 2 and 3 samples."""
    r = cc.MAX_TAPS // 2
    line = np.float32([3.0, 5.0, 11.0][:n])
    ext = _walked_extension(line, r)
    assert len(ext) == n + 2 * r
    np.testing.assert_array_equal(line[cc.mirror_index(np.arange(-r, n + r), n)], ext)
    if n == 3:
        np.testing.assert_array_equal(ext[r - 5:r], np.float32([5, 3, 5, 11, 5]))   # ... 1 0 1 2 1 | 0 1 2
    # and ref_pass reads through it, along every axis
    sigma = cc.sigma_for_taps(cc.MAX_TAPS)
    k = cc.taps(sigma)
    for axis in range(3):
        shape = [1, 1, 1]
        shape[2 - axis] = n
        out = cc.ref_pass(line.reshape(shape), sigma, axis).reshape(-1)
        for i in range(n):
            acc = np.float32(0)
            for j in range(len(k)):
                acc = cc.fma32(ext[i + j], k[j], acc)
            assert out[i] == acc


# ------------------------------------------------------------------ sigma_for_taps
def _cxx_taps(sigma):
    """gaussian_taps / check_content_sigmas of csrc/content_weights.hip: max(3, 2 * int(3 sigma + 0.5) + 1)."""
    return max(3, 2 * int(3 * sigma + 0.5) + 1)


def test_sigma_for_taps_gives_the_counts_the_cases_name():
    for K in cc.TAP_COUNTS + (cc.MAX_TAPS, cc.MAX_TAPS + 2):
        s = cc.sigma_for_taps(K)
        assert len(gaussian_kernel_1d(s, True)) == K and len(cc.taps(s)) == K and _cxx_taps(s) == K
    for s, K in zip((cc.SEAM_S1[0], cc.SEAM_S2[0]), cc.SEAM_TAPS):
        assert len(cc.taps(s)) == K and _cxx_taps(s) == K
    # 465 is the first count the limit refuses
    assert all(_cxx_taps(cc.sigma_for_taps(K)) <= cc.MAX_TAPS for K in range(3, cc.MAX_TAPS + 1, 2))
    assert _cxx_taps(cc.sigma_for_taps(cc.MAX_TAPS + 2)) == cc.MAX_TAPS + 2 > cc.MAX_TAPS
    # every case stays inside it, and taps are positive, symmetric and of sum about 1
    for name, c in cc.CASES.items():
        for s in c.s1 + c.s2:
            k = cc.taps(s)
            assert 3 <= len(k) <= cc.MAX_TAPS and np.all(k > 0) and np.array_equal(k, k[::-1]), name
            assert abs(float(k.astype(np.float64).sum()) - 1) < 1e-5


def test_tap_rotation_puts_every_count_on_every_slot():
    """Six different counts per case; over the eight cases every count once in each of the
    slots (s1x, s1y, s1z, s2x, s2y, s2z); the chunk structure the counts are there for."""
    rows = [cc.rotation_taps(r) for r in range(len(cc.TAP_COUNTS))]
    assert all(len(set(row)) == 6 for row in rows)
    for slot in range(6):
        assert sorted(row[slot] for row in rows) == sorted(cc.TAP_COUNTS)
    for r, row in enumerate(rows):
        c = cc.CASES[f"taps_r{r}"]
        assert [len(cc.taps(s)) for s in c.s1 + c.s2] == row
    chunks = lambda K: -(-K // cc.CHUNK)
    assert [chunks(K) for K in cc.TAP_COUNTS] == [1, 1, 1, 2, 2, 3, 3, 4]
    assert [chunks(K) for K in cc.SEAM_TAPS] == [2, 3] and chunks(cc.MAX_TAPS) == 29


# ------------------------------------------------------------------ mutants
SEAM_NAMES = [cc.seam_name(a, n) for a in range(3) for n in cc.SEAM_LENGTHS]
TAP_NAMES = [f"taps_r{r}" for r in range(len(cc.TAP_COUNTS))]


def _mutated(name, one_pass=cc.ref_pass, swap=None):
    c = cc.CASES[name]
    s1, s2 = (c.s1, c.s2) if swap is None else swap(c.s1, c.s2)
    return cc.ref_weights(cc.image(name), s1, s2, one_pass)


def _changed(name, **kw):
    return float(np.mean(_mutated(name, **kw) != cc.weights(name)))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_mutant_halo_not_fetched_across_a_seam(axis):
    """A pass along ``axis`` that takes 0 for the operands lying in a neighbouring 128-output
    tile: changes the 129 and 257 cases of that axis, and none of the shorter ones."""
    def one_pass(img, sigma, ax):
        if ax != axis:
            return cc.ref_pass(img, sigma, ax)
        return cc.ref_pass(img, sigma, ax, keep=lambda i, s: (s // cc.TILE == i // cc.TILE) | (s < 0) | (s >= len(i)))
    for n in cc.SEAM_LENGTHS:
        changed = _changed(cc.seam_name(axis, n), one_pass=one_pass)
        assert (changed > 0) == (n > cc.TILE), (axis, n, changed)
    # (a min or max that moved changes every voxel; otherwise at least the lines near the seam)


def _with_taps(edit):
    def one_pass(img, sigma, axis):
        k = cc.taps(sigma).copy()
        edit(k)
        return cc.ref_pass(img, sigma, axis, k=k)
    return one_pass


def test_mutant_last_tap_dropped():
    def edit(k):
        k[-1] = 0
    for name in TAP_NAMES + ["taps_max_s1", "taps_max_s2", cc.seam_name(1, 129)]:
        assert _changed(name, one_pass=_with_taps(edit)) > 0.5, name


def test_mutant_tail_chunk_dropped():
    """The ``if (kc < kpad)`` step left out: with an odd number of 16-tap chunks the taps of
    the last chunk are never applied.  Every tap case holds a count with an odd number of
    chunks (3, 5, 15: one; 33, 47: three), the 37-tap seam blur has three, 463 taps 29."""
    def edit(k):
        chunks = -(-len(k) // cc.CHUNK)
        if chunks % 2 == 1:
            k[cc.CHUNK * (chunks - 1):] = 0
    for name in TAP_NAMES + ["taps_max_s1", "taps_max_s2", cc.seam_name(2, 129)]:
        assert _changed(name, one_pass=_with_taps(edit)) > 0.5, name
    # and a count with an even number of chunks alone would not see it
    k = cc.taps(cc.sigma_for_taps(17)).copy()
    edit(k)
    np.testing.assert_array_equal(k, cc.taps(cc.sigma_for_taps(17)))


def test_mutant_unfused_multiply_add():
    """acc + v * k with a rounded product in place of the fused multiply-add: the last bits
    of a good part of the voxels, not of a stray one."""
    unfused = lambda img, sigma, axis: cc.ref_pass(img, sigma, axis, fma=lambda v, k, acc: acc + v * k)
    for name in TAP_NAMES + [cc.seam_name(0, 129)]:
        assert _changed(name, one_pass=unfused) > 0.1, name


def test_mutant_swapped_sigmas():
    """sigma1 and sigma2 exchanged, and two axes exchanged within both."""
    def axes(a, b):
        def swap(s1, s2):
            p = list(range(3))
            p[a], p[b] = p[b], p[a]
            return tuple(s1[i] for i in p), tuple(s2[i] for i in p)
        return swap
    for r, name in enumerate(TAP_NAMES):
        assert len(set(cc.rotation_taps(r))) == 6          # no two slots alike: every exchange is one
        assert _changed(name, swap=lambda s1, s2: (s2, s1)) > 0.5, name
        a, b = ((0, 1), (1, 2), (0, 2))[r % 3]
        assert _changed(name, swap=axes(a, b)) > 0.5, (name, a, b)


def _mirror_double(i, n):
    """The fold off by one: the end sample repeated (period 2 n)."""
    j = np.mod(np.asarray(i, np.int64), 2 * n)
    return np.where(j >= n, 2 * n - 1 - j, j)


def test_mutant_mirror_off_by_one_at_the_fold():
    other = lambda img, sigma, axis: cc.ref_pass(img, sigma, axis, source=_mirror_double)
    for name in SEAM_NAMES + ["taps_r0", "taps_max_s1", "taps_max_s2", "red_2", "red_30"]:
        assert _changed(name, one_pass=other) > 0, name


# ------------------------------------------------------------------ the reduction
def test_reduction_cases_place_the_extrema_where_they_can_be_missed():
    """red_tail: the maximum lies in the n % 256 voxels after the last whole block;
    red_second_round: the minimum lies past the first 1024 x 256 voxels; both extrema of
    both cases are unique, so missing one cannot be masked by a tie; the small cases have
    fewer voxels than one block."""
    r = cc.raw("red_tail")
    n = r.size
    assert cc.RED_ROUND < n < cc.RED_ROUND + 8192 and n % cc.RED_BLOCK != 0
    assert int(r.argmax()) >= n - n % cc.RED_BLOCK
    assert np.unravel_index(int(r.argmax()), r.shape) == cc.CASES["red_tail"].bead_at
    r2 = cc.raw("red_second_round")
    assert 2 * cc.RED_ROUND <= r2.size < 2 * cc.RED_ROUND + 8192
    assert int(r2.argmin()) >= cc.RED_ROUND
    for a in (r, r2):
        assert np.isfinite(a).all()
        assert (a == a.max()).sum() == 1 and (a == a.min()).sum() == 1
    # an extremum that is missed changes the weights
    for a, skip in ((r, slice(n - n % cc.RED_BLOCK, None)), (r2, slice(cc.RED_ROUND, None))):
        flat = a.reshape(-1)
        seen = np.delete(flat, np.arange(flat.size)[skip])
        assert (seen.min(), seen.max()) != (flat.min(), flat.max())
    assert [cc.raw(name).size for name in ("red_1", "red_2", "red_30")] == [1, 2, 30]
    assert cc.weights("red_1") is cc.raw("red_1")                 # range 0: skipped
    for name in ("red_2", "red_30"):
        w = cc.weights(name)
        assert w.min() == 0.0 and w.max() == 1.0 and (w == 0).sum() == 1 and (w == 1).sum() == 1


# ------------------------------------------------------------------ non-finite input
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_nonfinite_boxes_fit_and_bound_the_true_footprint(value):
    """The box that may hold NaN touches no border, so no fold brings it back in; with all
    the taps and none of the padding, the non-finite voxels are exactly the inner box, the
    range is NaN and the normalisation is skipped."""
    shape, at = cc.CASES["nonfinite"].shape, cc.NONFINITE_AT
    assert cc.NONFINITE_INNER == 2 and cc.NONFINITE_OUTER == 2 + 2 * (cc.CHUNK - 1)
    assert all(a - cc.NONFINITE_OUTER >= 1 and a + cc.NONFINITE_OUTER <= n - 2 for a, n in zip(at, shape))
    assert [len(cc.taps(s)) for s in cc.RED_SIGMA] == [3, 3, 3]
    inner, outer = cc.box(shape, at, cc.NONFINITE_INNER), cc.box(shape, at, cc.NONFINITE_OUTER)
    assert inner.sum() == 5 ** 3 and outer.sum() == 65 ** 3 and not outer.all()
    img = cc.nonfinite_volume(value)
    assert (~np.isfinite(img)).sum() == 1
    c = cc.CASES["nonfinite"]
    got = cc.ref_raw(img, c.s1, c.s2)
    np.testing.assert_array_equal(~np.isfinite(got), inner)
    np.testing.assert_array_equal(got[~inner], cc.raw("nonfinite")[~inner])
    assert np.isnan(got).any() and cr.normalize_image(got) is got
    assert cc.weights("nonfinite") is not cc.raw("nonfinite")     # (the clean image is normalised)


# ------------------------------------------------------------------ no subnormal intermediate
def test_no_intermediate_is_subnormal():
    """Every non-zero result of a multiply-add, the difference and the square stay above
    2^-100 in magnitude in every case: no flush-to-zero mode and no subnormal rounding can
    come between the kernels and the restatement.  Also: every value is finite."""
    floor = 2.0 ** -100
    lock = threading.Lock()
    smallest = [np.inf]

    def note(a):
        mag = np.abs(a)
        assert np.isfinite(mag).all()
        nz = mag[mag > 0]
        if nz.size:
            with lock:
                smallest[0] = min(smallest[0], float(nz.min()))

    def fma(v, k, acc):
        out = cc.fma32(v, k, acc)
        note(out)
        return out

    watched = lambda img, sigma, axis: cc.ref_pass(img, sigma, axis, fma=fma)
    for name, c in cc.CASES.items():
        trace = []
        cc.ref_raw(cc.image(name), c.s1, c.s2, watched, trace)
        assert len(trace) == 8
        for a in trace:
            note(a)
    print(f"smallest non-zero intermediate: 2^{np.log2(smallest[0]):.1f}")
    assert smallest[0] >= floor
