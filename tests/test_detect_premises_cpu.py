"""CPU: what tests/test_gpu_detect_edges.py relies on, proved from the references
(oracle/dog_ref.py, tests/detect_cases.py) and the tile sizes the library reports
(spim_detect_tiles) alone: the reference is the reference's per-voxel walk, and every case
hits the seam, the buffer fill, the capacity or the branch of the fit that its name says.
A case that stops doing so fails here, without a GPU."""
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc
from oracle import dog_ref
from spim_registration_amd import _lib, detect

NAN = float("nan")


@pytest.fixture(scope="module")
def t(lib):
    return detect.tiles()


def test_tiles_are_reported_and_the_cases_fit_them(t):
    assert all(v > 0 for v in t) and t.columns <= 62 and t.buffer >= t.columns
    # the fixed shapes of the value / NaN cases hold two strips, two row blocks and two chunks
    assert dc.wave_counts(dc.VALUE_SHAPE, t)[:3] == (2, 2, 2)
    assert all(np.prod(s) <= 110_000 for s, _, _ in dc.DENSE_CASES)


# ------------------------------------------------------------------ the reference
def special_volumes():
    rng = np.random.default_rng(5)
    a = np.round(rng.random((5, 6, 7)) * 3).astype(np.float32)            # plateaus and ties
    b = dc.noise((5, 5, 6), 6).copy()
    b[2, 2, 2], b[1, 3, 4], b[0, 0, 0] = np.nan, np.inf, np.nan
    b[3, 1, 1] = -np.inf
    c = np.where(rng.random((4, 5, 5)) < 0.5, np.float32(0.0), np.float32(-0.0))
    d = (rng.integers(1, 1 << 23, (5, 5, 5), dtype=np.uint32) | (rng.integers(0, 2, (5, 5, 5), dtype=np.uint32) << 31)) \
        .view(np.float32).copy()
    d[2, 2, 2], d[1, 1, 3] = 2.0 ** -126, -2.0 ** -125
    e = np.full((4, 4, 5), 1.5, np.float32)
    return [a, b, c, d, e]


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("T", [1, 3, 8])
def test_find_peaks_is_the_per_voxel_walk(k, T):
    """dog_ref.find_peaks against findPeaks / isSpecialPoint walked literally, on volumes with
    NaN, +-0, denormals, +-inf and plateaus, at thresholds that cut, at 0, at -0 and at NaN."""
    img = special_volumes()[k]
    mins = [0.0, -0.0, NAN, float(np.float32(2.0 ** -126)), 0.5, 1.0, float(np.inf)]
    n = 0
    for mv in mins:
        got = dog_ref.find_peaks(img, mv, T)
        want = dc.literal_peaks(img, mv, T)
        assert [g[:3] + g[4:] for g in got] == [w[:3] + w[4:] for w in want]
        np.testing.assert_array_equal(np.float32([g[3] for g in got]).view(np.uint32),
                                      np.float32([w[3] for w in want]).view(np.uint32))
        n += len(got)
    assert n > 0
    # the NaN threshold skips nothing; |v| >= NaN would skip everything
    assert dog_ref.find_peaks(img, NAN, T) == dog_ref.find_peaks(img, -1.0, T)


def test_denormals_are_not_flushed_here():
    img = dc.denormal_volume()
    assert np.count_nonzero(np.abs(img) < dc.F32_MIN_NORMAL) > 0.99 * img.size and not np.any(img == 0)
    all_ = dc.ref_peaks(img, 0.0)
    normal = dc.ref_peaks(img, float(dc.F32_MIN_NORMAL))
    # a flushing build sees one plateau of zeros with a few normal values: far more extrema
    flushed = dc.ref_peaks(np.where(np.abs(img) < dc.F32_MIN_NORMAL, np.float32(0), img), 0.0)
    assert 1000 < len(all_) < len(flushed) // 4 and 0 < len(normal) < 40
    assert all(p[3] >= dc.F32_MIN_NORMAL for p in normal)


# ------------------------------------------------------------------ a. dense seams
def test_dense_cases_cover_the_issue_lists(t):
    shapes = [s for s, _, _ in dc.DENSE_CASES]
    assert {s[2] for s in shapes} == set(dc.DENSE_NX) and {s[1] for s in shapes} == set(dc.DENSE_NY)
    assert {s[0] for s in shapes} == set(dc.DENSE_NZ) and (69, 7, 127) in shapes
    assert {T for _, T, _ in dc.DENSE_CASES} == set(dc.DENSE_T)
    assert any(s[2] < T for s, T, _ in dc.DENSE_CASES) and any(T > 1 and s[2] > T for s, T, _ in dc.DENSE_CASES)
    # every residue of the ring tail, in a first and in a last chunk
    assert set().union(*(dc.ring_residues(s, t) for s in shapes)) == {0, 1, 2}
    assert {(s[0] - 2) % t.planes % 3 for s in shapes if s[0] - 2 > t.planes} == {0, 1, 2}
    # a last wave with one tested column, one row, one centre plane
    assert any((s[2] - 2) % t.columns == 1 for s in shapes) and any((s[1] - 2) % t.rows == 1 for s in shapes)
    assert any((s[0] - 2) % t.planes == 1 for s in shapes)


@pytest.mark.parametrize("shape,T,seed", dc.DENSE_CASES)
def test_dense_candidates_sit_on_every_seam(t, shape, T, seed):
    peaks = dc.ref_peaks(dc.dense_volume(shape, seed), 0.0, True, True, T)
    assert any(p[4] for p in peaks) or len(peaks) < 3
    nz, ny, nx = shape
    for axis, n, tile in ((0, nx, t.columns), (1, ny, t.rows), (2, nz, t.planes)):
        have = {p[axis] for p in peaks}
        for c in [1, n - 2] + dc.seam_coordinates(n, tile):
            assert c in have, (axis, c)
    if T > 1 and nx > T:      # the x % T order is not the flat order
        assert [p[:3] for p in peaks] != sorted((p[:3] for p in peaks), key=lambda q: (q[2], q[1], q[0]))


def test_the_big_dense_case_has_every_seam(t):
    assert dc.seam_coordinates(127, t.columns) == [62, 63, 124, 125] and dc.seam_coordinates(7, t.rows) == [4, 5]
    assert dc.seam_coordinates(69, t.planes) == [64, 65]


# ------------------------------------------------------------------ b. block counts
def test_block_counts(t):
    got = [dc.wave_counts(dc.block_shape(g, t), t) for g in dc.BLOCK_GRIDS]
    assert tuple(w[4] for w in got) == dc.BLOCK_COUNTS
    assert all(w[3] % 4 != 0 for w in got)
    for g in dc.BLOCK_GRIDS:      # every wave has candidates: a wave run twice or not at all shows
        shape = dc.block_shape(g, t)
        assert np.prod(shape) <= 110_000
        peaks = dc.ref_peaks(dc.dense_volume(shape, dc.BLOCK_SEED), 0.0)
        assert {dc.wave_of(p, shape, t) for p in peaks} == set(range(dc.wave_counts(shape, t)[3]))


# ------------------------------------------------------------------ c. the candidate buffer
def test_buffer_fills(t):
    cases = dc.buffer_cases(t)
    trace = {}
    for name, (img, mp) in cases.items():
        peaks = dc.ref_peaks(img, mp, False, True)
        assert all(p[5] and not p[4] for p in peaks)
        trace[name] = dc.buffer_trace(peaks, img.shape, t)
    nz, ny, nx = cases["constant"][0].shape
    assert len(dc.ref_peaks(cases["constant"][0], 0.0, False, True)) == (nz - 2) * (ny - 2) * (nx - 2)
    fills, flushes = trace["constant"][0]
    assert set(fills) == {t.columns} and max(flushes.values()) == t.rows and min(flushes.values()) == t.rows - 1
    assert len(trace["constant"]) == 4      # two strips x two row blocks
    assert trace["exactly_full"] == {0: ([t.columns, t.buffer], {})}
    assert trace["one_more"] == {0: ([t.columns, t.buffer, 1], {1: 1})}
    assert trace["one_short_then_two"] == {0: ([t.columns, t.buffer - 1, 2], {1: 1})}


# ------------------------------------------------------------------ d. capacity
def test_capacity_counts(t):
    nz, ny, nx = dc.CAP_SHAPE
    assert (nz - 2) * (ny - 2) * (nx - 2) == t.cap_floor + 4 and nz * ny * nx // 256 < t.cap_floor
    for lowered, n in ((0, t.cap_floor + 4), (3, t.cap_floor + 1), (4, t.cap_floor), (5, t.cap_floor - 1)):
        assert len(dc.ref_peaks(dc.capacity_volume(lowered), 0.0, False, True)) == n
    assert 0 < len(dc.ref_peaks(dc.dense_volume(dc.CAP_SMALL_SHAPE, dc.CAP_SMALL_SEED), 0.0)) < 100


# ------------------------------------------------------------------ e. values
def test_value_cases(t):
    z = dc.zeros_volume()
    assert 0.4 < np.signbit(z).mean() < 0.6
    nz, ny, nx = z.shape
    pk = dc.ref_peaks(z, 0.0)
    assert len(pk) == (nz - 2) * (ny - 2) * (nx - 2) and all(p[5] and not p[4] for p in pk)
    assert not np.signbit(np.float32([p[3] for p in pk])).any()
    inf = dc.inf_volume()
    pk = dc.ref_peaks(inf, 0.0)
    kinds = {(p[4], p[5]) for p in pk if np.isinf(p[3])}
    assert kinds == {(True, False), (False, True)}      # +inf a MIN, -inf a MAX
    img, want = dc.plateau_volume(t)
    got = {p[:3]: (p[4], p[5]) for p in dc.ref_peaks(img, 0.0)}
    for v, kind in want.items():
        assert got.get(v) == kind, v
    sx, sy, sz = dc.seam_corner(t)
    assert len({dc.wave_of((sx + a, sy + b, sz + c), img.shape, t) for a in (0, 1) for b in (0, 1) for c in (0, 1)}) == 8
    for a, b in (((sx - 1, 2, 10), (sx + 1, 2, 10)), ((10, sy - 1, 20), (10, sy + 1, 20)), ((20, 2, sz - 1), (20, 2, sz + 1))):
        assert a in want and b in want and dc.wave_of(a, img.shape, t) != dc.wave_of(b, img.shape, t)
    c = img[41, sy, 41]       # the centre of the constant block: every neighbour equal
    assert np.all(img[40:43, sy - 1:sy + 2, 40:43] == c)


def test_threshold_at_a_candidate(t):
    img = dc.dense_volume(*dc.DENSE_CASES[4][::2])
    pk = dc.ref_peaks(img, 0.0)
    v = np.float32(sorted(p[3] for p in pk)[len(pk) // 2])
    at, above = dc.ref_peaks(img, float(v)), dc.ref_peaks(img, float(np.nextafter(v, np.float32(2))))
    assert len(at) == len(above) + 1 and 10 < len(above) < len(pk) - 10


# ------------------------------------------------------------------ f. NaN placement
def test_nan_cases(t):
    pos = dc.nan_positions(t)
    shape = dc.NAN_SHAPE
    x, y, z = pos["halo_column"]
    assert dc.wave_of((x - 1, y, z), shape, t) == 0 and dc.wave_of((x, y, z), shape, t) == 1
    x, y, z = pos["halo_row"]
    nsx = dc.wave_counts(shape, t)[0]
    assert dc.wave_of((x, y - 1, z), shape, t) == 0 and dc.wave_of((x, y, z), shape, t) == nsx
    x, y, z = pos["halo_plane"]
    assert dc.wave_of((x, y, z - 1), shape, t) == 0 and dc.wave_of((x, y, z), shape, t) == dc.wave_counts(shape, t)[3] // 2
    for name, p in pos.items():
        img = dc.nan_volume(p)
        assert np.isnan(img).sum() == 1 and np.isnan(img[p[2], p[1], p[0]])
        ref = {q[:3] for q in dc.ref_peaks(img, 0.0)}
        drop = dc.peaks_dropping_nan(img, 0.0)
        near = {(p[0] + a, p[1] + b, p[2] + c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)}
        assert not (ref & near) and ref < drop and (drop - ref) <= near
        # on each plane of the NaN's neighbourhood inside the image a dropped NaN shows
        planes = {q[2] for q in drop - ref}
        assert planes == {zz for zz in (p[2] - 1, p[2], p[2] + 1) if 1 <= zz <= shape[0] - 2}, name
    x, y, z = pos["mid_plane"]
    ref = dc.ref_peaks(dc.nan_volume(pos["mid_plane"]), 0.0)
    w = dc.wave_of((x, y, z), shape, t)
    assert {q[2] for q in ref if dc.wave_of(q, shape, t) == w} >= {z - 2, z - 1, z, z + 1, z + 2}


# ------------------------------------------------------------------ g. localisation
def test_the_trace_is_the_oracle_fit():
    for key in dc.LOC_VOLUMES:
        peaks, fitted = dc.expected_points(key)
        res, ends = dc.fit_trace(dc.LOC_VOLUMES[key](), peaks)
        assert len(res) == len(fitted) == len(peaks) > 0
        np.testing.assert_array_equal(np.float32(res).view(np.uint32), np.float32(fitted).view(np.uint32))


def test_integer_noise_takes_every_end_of_the_fit():
    peaks, fitted = dc.expected_points("int")
    _, ends = dc.fit_trace(dc.loc_int_volume(), peaks)
    assert len(peaks) > 300
    assert ends.count(dc.SINGULAR) >= 1 and ends.count(dc.BORDER) >= 1 and ends.count(dc.EXHAUSTED) >= 1
    stable = [e for e in ends if isinstance(e, int)]
    assert 1 in stable and 2 in stable and any(3 <= e <= dog_ref.MAX_NUM_MOVES for e in stable)
    assert dog_ref.MAX_NUM_MOVES + 1 in stable and max(stable) == dog_ref.MAX_NUM_MOVES + 1
    # an unstable fit keeps the integer position and |v|
    for pk, f, e in zip(peaks, fitted, ends):
        if not isinstance(e, int):
            assert tuple(float(v) for v in f) == (pk[0], pk[1], pk[2], pk[3])


def test_the_other_localisation_volumes():
    peaks, fitted = dc.expected_points("const")
    _, ends = dc.fit_trace(dc.loc_const_volume(), peaks)
    assert len(peaks) == 6 ** 3 and set(ends) == {dc.SINGULAR}
    peaks, fitted = dc.expected_points("float")
    _, ends = dc.fit_trace(dc.loc_float_volume(), peaks)
    assert len(peaks) > 1000 and sum(isinstance(e, int) for e in ends) > len(ends) // 2
    peaks, fitted = dc.expected_points("nonfinite")
    values = np.float32([f[3] for f in fitted])
    assert np.isnan(values).sum() >= 2 and np.isfinite(values).sum() > 100
    assert len(dc.select(peaks, fitted, 0.0)) == np.count_nonzero(np.abs(values) > 0)    # NaN fits are dropped


def test_selection_threshold_cases():
    peaks, fitted = dc.expected_points("float")
    values = np.abs(np.float32([f[3] for f in fitted]))
    med = np.float32(np.median(values))
    kept = dc.select(peaks, fitted, med)
    assert 0.4 * len(peaks) < len(kept) < 0.6 * len(peaks)
    v = values[values > med].min()      # a fitted |value|: at it the point goes, one ulp below it stays
    assert len(dc.select(peaks, fitted, v)) == len(dc.select(peaks, fitted, np.nextafter(v, np.float32(0)))) - 1
    below = float(v) * (1 - 2.0 ** -40)
    assert below < float(v) and np.float32(below) == v     # a double just below rounds to the float itself


# ------------------------------------------------------------------ the host-side argument rules
def test_argument_rules_need_no_gpu(lib):
    img = np.zeros(27, np.float32)
    dims = (C.c_int64 * 3)(3, 3, 3)
    n = C.c_int64(-1)
    pk = (_lib.Peak * 4)()
    ip = (_lib.InterestPointC * 4)()
    ptr = C.c_void_p(img.ctypes.data)

    def peaks(img=ptr, dims=dims, T=8, route=0, out=n):
        return lib.spim_detect_peaks(img, dims, 0.0, 1, 1, T, route, 0, pk, 4, C.byref(out) if out is not None else None)

    def points(loc=0, T=8, route=0):
        return lib.spim_detect_interest_points(ptr, dims, 0.0, 1, 1, T, route, 0, loc, 0.0, ip, 4, C.byref(n))
    big = (C.c_int64 * 3)(1 << 20, 1 << 10, 2)          # 2^31 voxels: 8 GiB
    for call, word in ((lambda: peaks(img=None), "null"), (lambda: peaks(dims=None), "null"),
                       (lambda: peaks(out=None), "null"), (lambda: peaks(dims=(C.c_int64 * 3)(3, 0, 3)), "dims"),
                       (lambda: peaks(T=0), "ij_threads"), (lambda: peaks(route=3), "route"),
                       (lambda: peaks(route=-1), "route"), (lambda: points(loc=2), "localization"),
                       (lambda: points(T=0), "ij_threads"), (lambda: points(route=7), "route"),
                       (lambda: peaks(dims=big, route=1), "4 GiB"),
                       (lambda: peaks(dims=(C.c_int64 * 3)(1 << 20, 1 << 20, 2)), "too large")):
        assert call() == -1 and word in _lib.last_error(), (word, _lib.last_error())
    assert n.value == -1
