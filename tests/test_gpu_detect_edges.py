"""The detection stage of csrc/detect.hip on a caller's image (spim_detect_peaks /
spim_detect_interest_points), at its edges: the seams of k_dog_peaks' waves, rows, z chunks
and load ring, its block remap, the per-wave candidate buffer, the capacity rerun, the
x % T sort, the values that decide ties, NaN on every halo, and each way the quadratic fit
ends.  Every case demands the exact ordered list (x, y, z, is_min, is_max) and the
intensities bit for bit, from k_dog_peaks and k_peaks_append alike, from a host pointer and
from a device tensor (left unchanged).  The references: oracle/dog_ref.py through
tests/detect_cases.py; that each case hits what its name says is proved on the CPU in
tests/test_detect_premises_cpu.py.
"""
import functools

import numpy as np
import pytest
import torch  # before the library loads: one shared HIP runtime (spim_registration_amd._lib.load)

import detect_cases as dc
from spim_registration_amd import _lib, detect, dog

pytestmark = pytest.mark.gpu

NAN = float("nan")
ROUTES = (detect.ROUTE_WAVE, detect.ROUTE_APPEND)


@functools.lru_cache(maxsize=None)
def tiles():
    return detect.tiles()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_peaks(got, exp):
    assert got.dtype == detect.PEAK_DTYPE
    want = np.array([(p[0], p[1], p[2], int(p[4]), int(p[5])) for p in exp], np.int64).reshape(-1, 5)
    have = np.stack([got[k].astype(np.int64) for k in ("x", "y", "z", "is_min", "is_max")], axis=1)
    assert len(have) == len(want), (len(have), len(want))
    np.testing.assert_array_equal(have, want)
    np.testing.assert_array_equal(bits(got["intensity"]), bits([p[3] for p in exp]))


def check(img, min_peak, find_min=True, find_max=True, T=8, routes=ROUTES):
    """Both candidate kernels, from the host array and from a device tensor, against
    detect_cases.ref_peaks.  Returns the expected list."""
    exp = dc.ref_peaks(img, min_peak, find_min, find_max, T)
    dev = torch.from_numpy(np.array(img)).cuda()
    for route in routes:
        for src in (img, dev):
            got = detect.peaks(src, min_peak, find_min, find_max, T, route, capacity=len(exp) + 8)
            assert_peaks(got, exp)
    np.testing.assert_array_equal(bits(dev.cpu().numpy()), bits(img))      # the input untouched
    return exp


def test_tiles_are_the_reported_constants(gpu):
    assert tiles() == (62, 4, 64, 64, 65536)


# ------------------------------------------------------------------ a. dense seams
@pytest.mark.parametrize("shape,T,seed", dc.DENSE_CASES)
def test_dense_noise_at_every_seam(gpu, shape, T, seed):
    """Float noise at threshold 0, both kinds: nx 3 .. 127 over the 62-column strips (a last
    wave with one column), ny 3 .. 11 over the 4-row blocks, nz 3 .. 69 over the 64-plane
    chunks and all three residues of the load ring's tail; T 1 .. 64 on either side of nx."""
    exp = check(dc.dense_volume(shape, seed), 0.0, T=T)
    assert len(exp) > 0
    one = check(dc.dense_volume(shape, seed), 0.0, find_min=False, T=T, routes=(detect.ROUTE_AUTO,))
    assert 0 < len(one) < len(exp) or len(exp) == 1


# ------------------------------------------------------------------ b. block counts
@pytest.mark.parametrize("grid,blocks", list(zip(dc.BLOCK_GRIDS, dc.BLOCK_COUNTS)))
def test_block_counts_and_the_xcd_remap(gpu, grid, blocks):
    """1, 7, 8, 9 and 15 blocks of four waves, the wave count no multiple of 4: the remap over
    8 XCDs with its remainder term, and the early return of the waves past the end."""
    t = tiles()
    shape = dc.block_shape(grid, t)
    assert dc.wave_counts(shape, t)[4] == blocks
    assert len(check(dc.dense_volume(shape, dc.BLOCK_SEED), 0.0)) > 10 * blocks


# ------------------------------------------------------------------ c. the candidate buffer
@pytest.mark.parametrize("name", ["constant", "exactly_full", "one_more", "one_short_then_two"])
def test_candidate_buffer_fills(gpu, name):
    """A wave's buffer filled by 62 per row with a flush per row (constant volume), filled to
    exactly 64 without a flush, to 64 then one more, and to 63 then two more."""
    img, min_peak = dc.buffer_cases(tiles())[name]
    exp = check(img, min_peak, find_min=False)
    assert len(exp) >= tiles().buffer
    check(img, min_peak)       # both kinds wanted: the same list (every candidate is a MAX)


# ------------------------------------------------------------------ d. capacity
def test_capacity_rerun_at_its_edge(gpu):
    """From a released workspace the capacity is the floor, 65536: 65537 maxima rerun the
    pass, 65536 do not, 65540 rerun it on the other kernel; then small calls meet the grown
    workspace.  Each route starts from a released workspace."""
    lib = _lib.load()
    floor = tiles().cap_floor
    small = dc.dense_volume(dc.CAP_SMALL_SHAPE, dc.CAP_SMALL_SEED)
    for route in ROUTES:
        for lowered, n in ((4, floor), (3, floor + 1), (0, floor + 4)):
            assert lib.spim_dog_release_workspace(0) == 0
            img = dc.capacity_volume(lowered)
            exp = dc.ref_peaks(img, 0.0, False, True)
            assert len(exp) == n
            got = detect.peaks(img, 0.0, False, True, 8, route, capacity=n)
            assert_peaks(got, exp)
            assert_peaks(detect.peaks(small, 0.0, True, True, 3, route), dc.ref_peaks(small, 0.0, T=3))
        # the capacity rule of the C ABI: the total is reported, the first `capacity` written
        short = detect.peaks(dc.capacity_volume(4), 0.0, False, True, 8, route, capacity=100)
        assert_peaks(short, dc.ref_peaks(dc.capacity_volume(4), 0.0, False, True))
    assert lib.spim_dog_release_workspace(0) == 0


# ------------------------------------------------------------------ e. values
def test_signed_zeros(gpu):
    """+0 and -0 mixed: every interior voxel has every neighbour >= it (a MAX), |v| = +0."""
    for min_peak in (0.0, -0.0):
        exp = check(dc.zeros_volume(), min_peak)
        assert not np.signbit(np.float32([p[3] for p in exp])).any()
    assert check(dc.zeros_volume(), float(np.float32(1e-45))) == []


def test_denormals_are_compared_as_they_are(gpu):
    """A volume of denormals: at min_peak 0 their extrema, at the smallest normal only those
    of the few normal values (a flushing build finds one plateau of zeros)."""
    img = dc.denormal_volume()
    assert len(check(img, 0.0)) > 1000
    assert 0 < len(check(img, float(dc.F32_MIN_NORMAL))) < 40


def test_infinities(gpu):
    exp = check(dc.inf_volume(), 0.0)
    assert np.isinf([p[3] for p in exp]).sum() >= 2
    assert all(np.isinf(p[3]) for p in check(dc.inf_volume(), float("inf")))


def test_plateaus_across_the_seams(gpu):
    """2 x 2 x 2 and 3 x 1 x 1 plateaus over a column, a row and a plane seam (>= and <= keep
    every voxel of them), and a constant block whose centre is both (the MAX wins)."""
    img, want = dc.plateau_volume(tiles())
    got = {p[:3]: (p[4], p[5]) for p in check(img, 0.0)}
    assert all(got[v] == kind for v, kind in want.items())
    const = np.full((7, 9, 66), -1.25, np.float32)
    assert all(p[5] and not p[4] for p in check(const, 0.0)) and check(const, 0.0, find_max=False) == []


def test_threshold_exactly_at_a_candidate_and_one_ulp_above(gpu):
    img = dc.dense_volume(*dc.DENSE_CASES[4][::2])
    pk = dc.ref_peaks(img, 0.0)
    v = np.float32(sorted(p[3] for p in pk)[len(pk) // 2])
    at = check(img, float(v))
    above = check(img, float(np.nextafter(v, np.float32(2))))
    assert len(at) == len(above) + 1


def test_nan_threshold_skips_nothing(gpu):
    """InteractiveIntegral.java:409 skips when |v| < minValue: false for a NaN minValue."""
    shape, T, seed = dc.DENSE_CASES[2]
    img = dc.dense_volume(shape, seed)
    assert check(img, NAN, T=T) == dc.ref_peaks(img, 0.0, T=T) != []


# ------------------------------------------------------------------ f. NaN placement
@pytest.mark.parametrize("name", ["halo_column", "halo_row", "halo_plane", "last_of_tiles", "face", "corner",
                                  "far_corner", "mid_plane"])
def test_one_nan(gpu, name):
    """One NaN whose 26 neighbours would each be an extremum if the NaN were dropped, on each
    halo of a wave, on the border, and inside a run of candidate planes: the wave's NaN
    ballot and its 3-plane window must send exactly these planes to the comparison loop."""
    pos = dc.nan_positions(tiles())[name]
    img = dc.nan_volume(pos)
    exp = check(img, 0.0)
    near = {(pos[0] + a, pos[1] + b, pos[2] + c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)}
    assert len(exp) > 1000 and not ({p[:3] for p in exp} & near)


# ------------------------------------------------------------------ g. localisation
def assert_points(got, peaks, fitted):
    """Interest points against (candidate, fit) pairs, positions and values bit for bit."""
    assert got.dtype == detect.IP_DTYPE and len(got) == len(peaks)
    want = np.float32([f[:3] for f in fitted]).reshape(-1, 3)
    pos32 = got["pos"].astype(np.float32)
    np.testing.assert_array_equal(pos32.astype(np.float64), got["pos"])     # floats stored as doubles
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(pos32), nan)
    np.testing.assert_array_equal(bits(np.where(nan, 0, pos32)), bits(np.where(nan, 0, want)))
    np.testing.assert_array_equal(bits(got["intensity"]), bits([f[3] for f in fitted]))
    np.testing.assert_array_equal(got["is_max"], [int(p[5]) for p in peaks])


def run_points(img, keep, localization=1, T=8):
    out = []
    dev = torch.from_numpy(np.array(img)).cuda()
    for route in ROUTES:
        for src in (img, dev):
            out.append(detect.interest_points(src, 0.0, localization, keep, True, True, T, route))
    np.testing.assert_array_equal(bits(dev.cpu().numpy()), bits(img))
    return out


@pytest.mark.parametrize("key", ["int", "float", "const"])
def test_quadratic_fit_bit_for_bit(gpu, key):
    """Every candidate's fit -- singular, off the border, out of moves, stable on pass 1 ..
    11 (integer noise), ordinary (float noise), all singular (constant) -- with nothing
    dropped (keep_threshold -1)."""
    peaks, fitted = dc.expected_points(key)
    for got in run_points(dc.LOC_VOLUMES[key](), -1.0):
        assert_points(got, peaks, fitted)
    # localisation 0 copies the candidates
    for got in run_points(dc.LOC_VOLUMES[key](), 0.0, localization=0):
        assert_points(got, peaks, [(p[0], p[1], p[2], p[3]) for p in peaks])


def test_fit_next_to_nan_and_inf(gpu):
    """Fits that read a NaN or an infinity come out NaN and fail ``|value| > threshold``; the
    rest stay, bit for bit and in order."""
    peaks, fitted = dc.expected_points("nonfinite")
    kept = dc.select(peaks, fitted, 0.0)
    assert 0 < len(kept) < len(peaks)
    for got in run_points(dc.loc_nonfinite_volume(), 0.0):
        assert_points(got, [k[0] for k in kept], [k[1] for k in kept])


def test_selection_threshold(gpu):
    """keep_threshold at the median (about half dropped, order kept), exactly at a fitted
    |value| (dropped), at a double just below it (the float rule: still dropped) and one
    float below (kept)."""
    peaks, fitted = dc.expected_points("float")
    values = np.abs(np.float32([f[3] for f in fitted]))
    med = np.float32(np.median(values))
    v = values[values > med].min()
    for thr in (float(med), float(v), float(v) * (1 - 2.0 ** -40), float(np.nextafter(v, np.float32(0)))):
        kept = dc.select(peaks, fitted, np.float32(thr))
        for got in run_points(dc.loc_float_volume(), thr):
            assert_points(got, [k[0] for k in kept], [k[1] for k in kept])
    assert len(dc.select(peaks, fitted, v)) + 1 == len(dc.select(peaks, fitted, np.nextafter(v, np.float32(0))))


def test_the_detectors_still_go_through_the_stage(gpu):
    """dog.simple_peaks equals the stage run on the DoG image it returns."""
    img = np.random.default_rng(3).random((20, 22, 70), dtype=np.float32)
    pts, d = dog.compute(img, threshold=0.0, find_min=True, return_dog=True, keep_intensity=True, ij_threads=3)
    got = detect.peaks(d, 0.0, True, True, 3)
    assert [tuple(int(c) for c in p.location) for p in pts] == [(int(g["x"]), int(g["y"]), int(g["z"])) for g in got]
    np.testing.assert_array_equal(bits([p.intensity for p in pts]), bits(got["intensity"]))
    assert_peaks(got, dc.ref_peaks(d, 0.0, T=3))
