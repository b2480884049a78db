"""CPU: the premises of tests/test_gpu_thinout.py -- the restatement in tests/thinout_ref.py is
what it says, the cases hold what the GPU tests rely on -- and the argument errors of
csrc/thinout.hip and of ``process_timepoint(thin_out=...)`` that need no device."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import thinout_ref as tr
from spim_registration_amd import _lib, pipeline, thinout

ERR_ARG = -1
BIG = [c for c in tr.SIZE_CASES if c[1] >= 16]


@functools.lru_cache(maxsize=None)
def case(seed, n, vox):
    return tr.make_case(seed, n, tr.VOXELS[vox])


@functools.lru_cache(maxsize=None)
def reference(seed, n, vox):
    return tr.nn_distances(case(seed, n, vox), tr.VOXELS[vox])


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("vox", sorted(tr.VOXELS))
def test_chunked_restatement_equals_a_plain_double_loop(vox):
    """also with chunks that do not divide n, on the lattice's ties and the seam case's twins"""
    lat = tr.lattice_case(4)
    for pts in (case(1, 2, vox), case(1, 3, vox), case(3, 97, vox), lat, tr.seam_case()[0][90:310]):
        want_d, want_i = tr.nn_distances_loop(pts, tr.VOXELS[vox])
        for chunk in (128, 7):
            d, i = tr.nn_distances(pts, tr.VOXELS[vox], chunk)
            np.testing.assert_array_equal(d.view(np.uint64), want_d.view(np.uint64))
            np.testing.assert_array_equal(i, want_i)
    d, i = tr.nn_distances(np.array([[1.0, 2.0, 3.0]]))
    assert np.isposinf(d).all() and list(i) == [-1]
    d, i = tr.nn_distances(np.zeros((0, 3)))
    assert len(d) == len(i) == 0


@pytest.mark.parametrize("vox", sorted(tr.VOXELS))
@pytest.mark.parametrize("seed,n", [c for c in tr.SIZE_CASES if c[1] <= tr.C_TILE + 1])
def test_root_of_the_minimum_is_the_minimum_of_the_roots(seed, n, vox):
    """sqrt(min s) == min sqrt(s) bitwise (a correctly rounded root is monotone), and the first
    index of the smallest root is no lower than that of the smallest sum's only where the roots
    of different sums coincide -- then the strict rule on s may name another point than a strict
    rule on the roots: the cases do not hold such a point"""
    c = tr.scaled(case(seed, n, vox), tr.VOXELS[vox])
    s = tr.pair_sums(c, c)
    s[np.arange(n), np.arange(n)] = np.inf
    roots = np.sqrt(s)
    d, i = reference(seed, n, vox)
    np.testing.assert_array_equal(roots.min(axis=1).view(np.uint64), d.view(np.uint64))
    np.testing.assert_array_equal(np.argmin(roots, axis=1), i)


def _rn(x: Fraction) -> float:
    return float(x)   # Fraction.__float__ rounds to nearest, ties to even


def _sums(a, b):
    """(the restated s of the pair, s with each addition fused with its right product, s with the
    first addition fused with its left product) in exact rational arithmetic"""
    d = [Fraction(_rn(Fraction(x) - Fraction(y))) for x, y in zip(a, b)]
    sq = [q * q for q in d]
    plain = _rn(Fraction(_rn(Fraction(_rn(sq[0])) + Fraction(_rn(sq[1])))) + Fraction(_rn(sq[2])))
    right = _rn(Fraction(_rn(Fraction(_rn(sq[0])) + sq[1])) + sq[2])
    left = _rn(Fraction(_rn(sq[0] + Fraction(_rn(sq[1])))) + sq[2])
    return plain, right, left


def test_a_fused_multiply_add_would_round_differently():
    """among the pairs (i, nearest[i]) of the anisotropic cases there are some whose distance a
    contracted evaluation changes, for either way of contracting: such a kernel cannot pass"""
    seed, n = 1, tr.R_BLOCK + 1
    c = tr.scaled(case(seed, n, "aniso"), tr.VOXELS["aniso"])
    d, i = reference(seed, n, "aniso")
    changed = {"right": 0, "left": 0}
    for k in range(n):
        plain, right, left = _sums(c[k], c[i[k]])
        assert np.sqrt(np.float64(plain)) == d[k]          # the rational chain is the restatement's
        changed["right"] += np.sqrt(np.float64(right)) != d[k]
        changed["left"] += np.sqrt(np.float64(left)) != d[k]
    assert changed["right"] >= 3 and changed["left"] >= 3, changed
    # and the scaling itself is inexact there: 0.73 is no dyadic rational
    p = case(seed, n, "aniso")
    assert any(Fraction(float(c[k, 0])) != Fraction(float(p[k, 0])) * Fraction(0.73) for k in range(n))


@pytest.mark.parametrize("vox", sorted(tr.VOXELS))
@pytest.mark.parametrize("seed,n", BIG)
def test_cases_hold_what_the_gpu_tests_rely_on(seed, n, vox):
    """duplicates (distance 0, the twin named), distances on both sides of both thresholds and
    one exactly on each"""
    d, i = reference(seed, n, vox)
    assert np.isfinite(d).all() and (i >= 0).all() and (i != np.arange(n)).all()
    assert (d == 0.0).sum() >= 2 * (n // 16)
    assert (d == tr.MIN_D).sum() == 2 and (d == tr.MAX_D).sum() == 2
    assert ((d > 0) & (d < tr.MIN_D)).any() and ((d > tr.MIN_D) & (d < tr.MAX_D)).any() and (d > tr.MAX_D).any()
    for keep_range in (False, True):
        k = tr.keep_flags(d, tr.MIN_D, tr.MAX_D, keep_range)
        assert 0 < k.sum() < n
        assert k[d == tr.MIN_D].all() == keep_range and k[d == tr.MAX_D].all() == keep_range
    both = tr.keep_flags(d, tr.MIN_D, tr.MAX_D, False) ^ tr.keep_flags(d, tr.MIN_D, tr.MAX_D, True)
    assert both.all()   # the two rules are complements for finite distances


def test_lattice_and_seam_cases_are_what_they_say():
    side = 6
    lat = tr.lattice_case(side)
    s, i = tr.nn_sums(lat)
    assert (s == 1.0).all()
    c = lat.astype(int)
    inner = ((c > 0) & (c < side - 1)).all(axis=1)
    assert inner.sum() == (side - 2) ** 3
    np.testing.assert_array_equal(i[inner], np.nonzero(inner)[0] - side * side)
    full = tr.pair_sums(lat, lat)
    assert ((full == 1.0).sum(axis=1)[inner] == 6).all()
    pts, want = tr.seam_case()
    assert len(pts) == 2 * tr.C_TILE
    d, i = tr.nn_distances(pts)
    for k, j in want.items():
        assert i[k] == j
    assert all(d[k] == 0.0 for k in (0, len(pts) - 1, 100, 300, 700))
    for k in (tr.R_BLOCK - 1, tr.R_BLOCK, tr.C_TILE - 1, tr.C_TILE):
        others = np.delete(np.arange(len(pts)), [k, want[k]])
        assert 0 < d[k] < 1.0 and np.sqrt(tr.pair_sums(pts[k:k + 1], pts[others])).min() > 50.0
    assert tr.SPLIT_N > 4 * tr.C_TILE and tr.SPLIT_CASE[1] < 400


# ---------------------------------------------------------------- the histogram's restatement
def test_histogram_restatement():
    d, _ = reference(1, tr.C_TILE + 1, "aniso")
    centres, counts, lo, hi = tr.histogram(d, bins=100)
    assert lo == d.min() == 0.0 and hi == d.max()
    assert counts.sum() == len(d) and counts[-1] >= 1
    size = (hi - lo) + 0.000001
    assert int(np.floor(((hi - lo) / size) * 100)) == 99           # the maximum: the last bin
    assert centres[0] == lo + (size / 100) / 2 and centres[99] == (lo + (size / 100) / 2) + (size / 100) * 99.0
    sel = np.random.default_rng(5).random(len(d)) < 1.0 / 3.0
    _, counts, lo, hi = tr.histogram(d, sel, bins=17)
    assert counts.sum() == sel.sum() and lo == d[sel].min() and hi == d[sel].max()
    # all distances equal: size = 0.000001, everything in bin 0
    centres, counts, lo, hi = tr.histogram(np.full(9, 2.5), bins=10)
    assert list(counts) == [9] + [0] * 9 and lo == hi == 2.5
    # max - min absorbs the 0.000001: Java's ArrayIndexOutOfBoundsException
    with pytest.raises(IndexError):
        tr.histogram(np.array([0.0, 1e12]), bins=100)


def test_subsampling_mask_is_numpy_s_draw():
    assert thinout.subsampling_mask(10, 1, seed=3) is None
    m = thinout.subsampling_mask(1000, 3, seed=3)
    np.testing.assert_array_equal(m, (np.random.default_rng(3).random(1000) < 1.0 / 3.0).astype(np.uint8))
    assert m.dtype == np.uint8 and 250 < m.sum() < 420
    with pytest.raises(ValueError):
        thinout.subsampling_mask(10, 0)


# ---------------------------------------------------------------- argument errors without a device
def test_header_defaults_and_tiles(lib):
    p = _lib.ThinOutParams()
    lib.spim_thinout_params_default(C.byref(p))
    assert (p.min_distance, p.max_distance, p.keep_range, p.t_split, p.device) == (0.0, 5.0, 0, 0, 0)
    assert C.sizeof(_lib.ThinOutParams) == 32
    assert thinout.tile_sizes() == (tr.R_BLOCK, tr.C_TILE)


def _thin(lib, p, n=4, compact=True):
    pts = np.arange(3.0 * n).reshape(n, 3)
    vox = np.ones(3)
    dist, nearest, kept = np.empty(n), np.empty(n, np.int32), np.empty(n, np.int32)
    count = C.c_int64(-7)
    args = [C.c_void_p(pts.ctypes.data), n, vox.ctypes.data_as(_lib._pd), C.byref(p), C.c_void_p(dist.ctypes.data),
            C.c_void_p(nearest.ctypes.data)]
    if compact:
        return lib.spim_thin_out(*args, C.c_void_p(kept.ctypes.data), n, C.byref(count))
    return lib.spim_nn_distances(*args)


@pytest.mark.parametrize("lo,hi", [(5.0, 5.0), (6.0, 5.0), (float("nan"), 5.0), (0.0, float("nan"))])
def test_min_not_below_max_is_an_argument_error(lib, lo, hi):
    p = _lib.ThinOutParams()
    lib.spim_thinout_params_default(C.byref(p))
    p.min_distance, p.max_distance = lo, hi
    for compact in (True, False):
        assert _thin(lib, p, compact=compact) == ERR_ARG
        assert lib.spimdecon_last_error().startswith(b"thinout: min_distance")
    with pytest.raises(ValueError, match="min_distance"):
        thinout.check_range(lo, hi)


def test_other_argument_errors(lib):
    p = _lib.ThinOutParams()
    lib.spim_thinout_params_default(C.byref(p))
    p.t_split = -1
    assert _thin(lib, p) == ERR_ARG and lib.spimdecon_last_error().startswith(b"thinout: t_split")
    d = np.array([1.0, 2.0, 3.0])
    lo, hi = C.c_double(), C.c_double()
    counts, centres = np.zeros(4, np.int64), np.zeros(4)

    def hist(n, bins):
        return lib.spim_distance_histogram(C.c_void_p(d.ctypes.data), n, None, bins, 0, C.byref(lo), C.byref(hi),
                                           counts.ctypes.data_as(_lib._pi64), centres.ctypes.data_as(_lib._pd))
    for bins in (0, -3):
        assert hist(3, bins) == ERR_ARG and lib.spimdecon_last_error().startswith(b"thinout: num_bins")
    assert hist(3, 4097) == ERR_ARG and lib.spimdecon_last_error().startswith(b"thinout: more than 4096 bins")
    for n in (0, 1):
        assert hist(n, 4) == ERR_ARG and lib.spimdecon_last_error().startswith(b"thinout: a histogram needs")
    with pytest.raises(ValueError, match="bins"):
        thinout.distance_histogram([np.zeros((3, 3))], (1, 1, 1), bins=0)
    with pytest.raises(ValueError, match="voxel_sizes"):
        thinout.distance_histogram([np.zeros((3, 3))], [(1, 1, 1), (1, 1, 2)])


class _NeverDetected(Exception):
    pass


class _Views:
    """stands in for the views: the keyword validation must be over before one is touched"""
    def __iter__(self):
        raise _NeverDetected()


@pytest.mark.parametrize("bad,match", [
    ({"min_distance": 5.0, "max_distance": 5.0}, "min_distance"),
    ({"min_distance": 6.0, "max_distance": 2.0}, "min_distance"),
    ({"min_distance": 0.0, "max_distance": 5.0, "keep": True}, "unknown keys"),
    ((0.0, 5.0), "dict"),
])
def test_pipeline_validates_thin_out_before_any_work(bad, match):
    with pytest.raises(ValueError, match=match):
        pipeline.process_timepoint(_Views(), [], (0, 0, 0), (8, 8, 8), thin_out=bad)
    with pytest.raises(ValueError, match=match):
        pipeline.Pipeline(thin_out=bad).process(_Views(), [], (0, 0, 0), (8, 8, 8))
    with pytest.raises(ValueError, match="voxel_size"):
        pipeline.process_timepoint(_Views(), [], (0, 0, 0), (8, 8, 8), thin_out={}, voxel_size=(1.0, 1.0))
