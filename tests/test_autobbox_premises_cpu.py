"""The premises of tests/test_gpu_autobbox_edges.py, proved without a GPU: the additive images
of tests/autobbox_cases.py decompose, so no pass hides behind another; every radius of the
sweep takes the tile class, the level count and the overlap shift the case list says; the
special values sit where the seams are; the box and min / max cases place their voxels where
they can be missed -- and the cases can tell the mistakes they are there for (a window one
short at a seam, a halo not fetched across a seam, the other class's seams, the overlap shift
off by one, the remainder of the 4-wide loop left out, a comparison that lets a NaN in)."""
import numpy as np
import pytest

import autobbox_cases as ac
import autobbox_ref as ar

u32 = ac.u32


def changed(c, **mutant):
    """the positions along the pass axis where the mutant of the pass differs from the pass"""
    a = ac.sweep_profiles(c.name)[c.axis]
    good = ac.window_min(a, c.r)
    bad = ac.tiled_pass(a, c.r, **mutant)
    return set(np.nonzero(u32(good) != u32(bad))[0].tolist()), a, good


# ------------------------------------------------------------------ the decomposition
DECOMPOSED = ac.RADIUS_SWEEP + ac.LENGTH_SWEEP[::4]


@pytest.mark.parametrize("name", [c.name for c in DECOMPOSED])
def test_additive_images_decompose(name):
    """ar.min_filter of a[x] + b[y] + c[z] is minwin(a)[x] + minwin(b)[y] + minwin(c)[z], bit for
    bit: every output voxel shows the window of every axis at its position, none is masked by
    another pass or by the zero extension (all values are negative)."""
    c = ac.SWEEPS[name]
    a, b, cz = ac.sweep_profiles(name)
    img = ac.sweep_image(name)
    assert img.shape == c.shape and img.max() < 0 and img.min() >= -3
    exact = (cz.astype(np.float64)[:, None, None] + b.astype(np.float64)[None, :, None]) + a.astype(np.float64)
    np.testing.assert_array_equal(img.astype(np.float64), exact)            # (every sum is exact)
    want = ac.additive(ac.window_min(a, c.r), ac.window_min(b, c.r), ac.window_min(cz, c.r))
    np.testing.assert_array_equal(u32(ac.sweep_expected(name)), u32(want))
    along = ac.sweep_profiles(name)[c.axis]
    assert len(np.unique(along)) >= len(along) // 2 and np.all(along[1:] != along[:-1])   # no repeated neighbours


def test_sweep_shapes_have_the_seams_they_name():
    for c in ac.SWEEPS.values():
        tile = ac.tile_of(c.r)
        nz, ny, nx = c.shape
        assert (nx, ny, nz)[c.axis] == c.n
        lines = ny * nz if c.axis == 0 else nx
        assert ac.LINES < lines < 2 * ac.LINES                    # two line groups, the second partial
    for c in ac.RADIUS_SWEEP:
        tile = ac.tile_of(c.r)
        assert c.n > 2 * tile and c.n % tile == 3                 # three tiles, the last of 3 outputs
        assert [kind for _, kind in ac.seams(c)] == ["falling", "rising"]
    assert {(c.axis, c.r) for c in ac.RADIUS_SWEEP} == {(a, r) for a in range(3) for r in ac.RADII}
    for axis in range(3):
        for r in ac.LENGTH_RADII:
            tile = ac.tile_of(r)
            ns = [c.n for c in ac.LENGTH_SWEEP if (c.axis, c.r) == (axis, r)]
            assert ns == [tile - 1, tile, tile + 1, tile + 2, tile + 3, 2 * tile, 2 * tile + 1]
            # four consecutive lengths: the staged length of the last tile, (tile | 1 | 2 | 3) + 2r, in every residue
            assert {(((n - 1) % tile + 1) + 2 * r) % ac.UNROLL for n in ns[1:5]} == {0, 1, 2, 3}
    assert max(int(np.prod(c.shape)) for c in ac.SWEEPS.values()) == 259 * 66 * 3


# ------------------------------------------------------------------ classes, levels and shifts
def test_every_radius_takes_the_class_the_list_says():
    assert tuple(sorted(ac.RADIUS_CLASSES)) == ac.RADII == (1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64)
    for r, (tile, levels, shift) in ac.RADIUS_CLASSES.items():
        w = 2 * r + 1
        lv, p, sh = ac.doubling(r)
        assert (ac.tile_of(r), lv, sh) == (tile, levels, shift)
        assert p <= w < 2 * p and 1 <= sh < p and p == 2 ** levels
        k, n_levels = 1, 0                  # the kernel's own loop: for (k = 1; 2 * k <= w; k *= 2)
        while 2 * k <= w:
            k, n_levels = 2 * k, n_levels + 1
        assert (n_levels, k, w - k) == (lv, p, sh)
    assert ac.tile_of(ac.SMALL_RADIUS) == ac.TILE_SMALL and ac.tile_of(ac.SMALL_RADIUS + 1) == ac.TILE_LARGE
    for j in range(1, 7):                   # the extremes of the shift and the step of the level count
        assert ac.doubling(2 ** j)[1:] == (2 ** (j + 1), 1) and 2 ** j in ac.RADII
        assert ac.doubling(2 ** j - 1)[1:] == (2 ** j, 2 ** j - 1) and 2 ** j - 1 in ac.RADII
        assert ac.doubling(2 ** j)[0] == ac.doubling(2 ** j - 1)[0] + 1


# ------------------------------------------------------------------ the tiled restatement and its mutants
def test_tiled_pass_is_the_window_minimum():
    """Without a mutant, tiled_pass is ar.min_filter_axis: on every sweep profile, with either
    tile (the class alone does not show in the result: the getter test is what pins it), and on
    lines of both signs with NaN, -0 and +Inf."""
    for c in ac.SWEEPS.values():
        diff, a, good = changed(c)
        assert not diff, c.name
        np.testing.assert_array_equal(u32(ac.tiled_pass(a, c.r, tile=ac.TILE_SMALL)), u32(good))
    rng = np.random.default_rng(1)
    lines = (rng.random((200, 7)) * 2 - 1).astype(np.float32)
    lines[50, 1], lines[60:64, 2], lines[62, 2], lines[100:140, 3] = np.nan, 0.0, -0.0, np.inf
    for r in (1, 3, 16, 17, 64):
        want = ar.min_filter_axis(lines.T.reshape(7, 1, 200), r, 2).reshape(7, 200).T
        np.testing.assert_array_equal(u32(ac.tiled_pass(lines, r)), u32(want))
        assert r > 17 or np.any(want == ar.FLOAT_MAX)


@pytest.mark.parametrize("name", list(ac.SWEEPS))
def test_seam_mutants_are_visible_at_the_seam(name):
    """A window one short on the left shows at the first output after every rising seam and
    nowhere else, one short on the right at the last output before every falling seam whose
    halo lies in the image; zeros for the halo show within r of every seam."""
    c = ac.SWEEPS[name]
    seams = ac.seams(c)
    left, _, _ = changed(c, left_short=True)
    assert left == {s for s, kind in seams if kind == "rising"}
    right, _, _ = changed(c, right_short=True)
    assert right == {s - 1 for s, kind in seams if kind == "falling" and s - 1 + c.r < c.n}
    halo, _, _ = changed(c, zero_halo=True)
    assert halo <= {i for s, _ in seams for i in range(s - c.r, s + c.r)}
    for s, kind in seams:
        assert (s if kind == "rising" else s - 1) in halo


def test_every_seam_mutant_is_caught_on_every_axis_at_every_radius():
    """what the parametrised test above leaves open: that the sets are not empty where it matters"""
    for axis in range(3):
        for r in ac.RADII:
            c = ac.SWEEPS[ac.Sweep(axis, r, 2 * ac.tile_of(r) + 3).name]
            tile = ac.tile_of(r)
            assert changed(c, left_short=True)[0] == {2 * tile}
            assert changed(c, right_short=True)[0] == {tile - 1}
            assert {tile - 1, 2 * tile} <= changed(c, zero_halo=True)[0]
        for r in ac.LENGTH_RADII:
            cases = [c for c in ac.LENGTH_SWEEP if (c.axis, c.r) == (axis, r)]
            assert sum(bool(changed(c, left_short=True)[0]) for c in cases) >= 1
            assert sum(bool(changed(c, right_short=True)[0]) for c in cases) >= 1
            assert sum(bool(changed(c, zero_halo=True)[0]) for c in cases) == 5      # every length past one tile


@pytest.mark.parametrize("c", [c for c in ac.RADIUS_SWEEP if c.axis == 0 and c.r > ac.SMALL_RADIUS],
                         ids=lambda c: c.name)
def test_the_small_tiles_seams_are_visible_at_a_large_radius(c):
    """A halo lost at the seams of the 64 tile changes a large-class case where the same
    mistake at the 128 seams does not: more than r from every seam of the large tile."""
    small, _, _ = changed(c, zero_halo=True, tile=ac.TILE_SMALL)
    large, _, _ = changed(c, zero_halo=True)
    assert small and large and small != large
    if c.r <= ac.TILE_SMALL // 2:
        assert any(all(abs(i - s) > c.r for s in range(0, c.n + 1, ac.TILE_LARGE)) for i in small)


@pytest.mark.parametrize("name", list(ac.SWEEPS))
def test_a_shift_off_by_one_is_visible(name):
    """shift - 1 leaves the last element out of every window: wrong wherever that element is
    the window's minimum, which is every output whose window lies on a falling slope (every
    radius has such a seam in the radius sweep)."""
    c = ac.SWEEPS[name]
    diff, a, good = changed(c, shift_off=-1)
    assert diff or c not in ac.RADIUS_SWEEP
    for i in diff:
        assert i + c.r < c.n and a[i + c.r] == good[i]
    for s, kind in ac.seams(c):
        if kind == "falling" and s - 1 + c.r < c.n:
            assert s - 1 in diff


def test_a_skipped_remainder_is_visible():
    """Leaving out the remainder of the 4-wide loop loses elements at the end of a tile's staged
    line: it shows in the last three outputs of a tile and nowhere else.  In a full tile that
    ends on a falling slope every radius shows it.  In the ragged last tile the
    staged end is the zero extension, which never wins in an additive image; only a level with
    k = r still loses the image's last element there (r = 16 and 64 at tile + 2) -- the positive
    images, where the zeros win, are for that tile (test_positive_images_show_the_ragged_tile)."""
    for c in ac.SWEEPS.values():
        tile = ac.tile_of(c.r)
        diff, _, _ = changed(c, skip_remainder=True)
        ends = {i for p0 in range(0, c.n, tile) for i in range(min(p0 + tile, c.n) - 3, min(p0 + tile, c.n)) if i >= p0}
        assert diff <= ends, c.name
    for c in ac.RADIUS_SWEEP:
        tile = ac.tile_of(c.r)
        diff, _, _ = changed(c, skip_remainder=True)
        assert diff & {tile - 3, tile - 2, tile - 1}, c.name
    for r in (16, 64):
        c = ac.SWEEPS[ac.Sweep(0, r, ac.tile_of(r) + 2).name]
        assert changed(c, skip_remainder=True)[0] == {c.n - 2}


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("r", ac.POSITIVE_RADII)
def test_positive_images_show_the_ragged_tile(r, axis):
    """A skipped remainder in the ragged last tile of 1, 2 or 3 outputs changes the filtered
    positive image in that tile, at two of the three lengths at least (at the third the loop
    has no remainder that an output reads); with one full tile it shows in that tile."""
    tile = ac.tile_of(r)
    seen = []
    for d in range(4):
        c = ac.POSITIVES[ac.Positive(axis, r, tile + d).name]
        img = ac.positive_image(c.name)
        want = ar.min_filter(img, r)
        np.testing.assert_array_equal(u32(ac.chain(img, r)), u32(want))
        assert img.min() >= 0.5 and (want > 0).any()
        bad = np.moveaxis(u32(ac.chain(img, r, axis, skip_remainder=True)) != u32(want), 2 - axis, 0)
        at = set(np.nonzero(bad.reshape(c.n, -1).any(axis=1))[0].tolist())
        assert at <= set(range(tile - 3, tile)) | set(range(tile, c.n))
        seen.append(bool(at & set(range(tile, c.n))) if d else bool(at))
    assert seen[0] and sum(seen[1:]) >= 2, seen


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_mutant_of_one_pass_changes_the_filtered_volume(axis):
    """The step from the line to the volume: the chain of three passes with one mutant pass
    differs from ar.min_filter in exactly the planes the line says."""
    c = ac.SWEEPS[ac.Sweep(axis, 17, 2 * ac.TILE_LARGE + 3).name]
    out = ac.chain(ac.sweep_image(c.name), c.r, axis, right_short=True)
    bad = np.moveaxis(u32(out) != u32(ac.sweep_expected(c.name)), 2 - axis, 0)
    assert set(np.nonzero(bad.reshape(c.n, -1).any(axis=1))[0].tolist()) == {ac.TILE_LARGE - 1}
    assert bad[ac.TILE_LARGE - 1].all()


# ------------------------------------------------------------------ special values
@pytest.mark.parametrize("name", list(ac.SPECIALS))
def test_special_values_straddle_the_seams(name):
    s = ac.SPECIALS[name]
    tile = ac.tile_of(s.r)
    img = ac.special_image(name)
    want = ar.min_filter(img, s.r)
    nan = np.isnan(want)
    for a in range(3):          # the NaN's footprint: both sides of the first seam of every axis
        idx = np.nonzero(nan.any(axis=tuple(b for b in range(3) if b != a)))[0]
        assert idx.min() == s.nan_at[a] - s.r < tile - 1 and tile <= idx.max() == min(s.nan_at[a] + s.r, s.side - 1)
    assert nan.sum() == np.prod([min(at + s.r, s.side - 1) - (at - s.r) + 1 for at in s.nan_at])
    assert np.unique(u32(want[nan])).size == 1
    z, y, x = s.zero_at
    assert x == tile - 1 and u32(img[z, y, x]) == 0 and u32(img[z, y, x + 1]) == 0x80000000
    row = want[z, y]            # -0 where the window reaches x + 1, +0 where it reaches x only
    assert np.all(u32(row[x + 1 - s.r:x + 2 + s.r]) == 0x80000000) and u32(row[x - s.r]) == 0
    assert row[x - s.r - 1] > 0 and (x + 2 + s.r >= s.side or row[x + 2 + s.r] > 0)
    ninf = want == -np.inf
    assert ninf.sum() == np.prod([min(at + s.r, s.side - 1) - (at - s.r) + 1 for at in s.ninf_at])
    assert ninf[:, :, :tile].any() and ninf[:, :, tile:].any()


@pytest.mark.parametrize("name", list(ac.INF_CASES))
def test_the_infinite_image_has_an_interior(name):
    shape, r = ac.INF_CASES[name]
    want = ar.min_filter(ac.inf_image(name), r)
    inner = tuple(slice(r, n - r) for n in shape)
    assert want[inner].size > 0 and np.all(want[inner] == ar.FLOAT_MAX)
    assert shape[2] - 2 * r > ac.tile_of(r)                      # the interior crosses an x seam
    rim = np.ones(shape, bool)
    rim[inner] = False
    assert np.all(u32(want[rim]) == 0)


# ------------------------------------------------------------------ the box
def test_every_planted_voxel_holds_one_face():
    full = ar.threshold_bounds(ac.faces_image(), ac.FACES_THRESHOLD)
    assert full[2] and int(np.prod(ac.FACES_SHAPE)) > ac.BOX_ROUND and ac.FACES_SHAPE[2] & (ac.FACES_SHAPE[2] - 1)
    for name in ac.FACES:
        lo, hi, found = ar.threshold_bounds(ac.faces_image(without=name), ac.FACES_THRESHOLD)
        moved = [f"{'xyz'[a]}min" for a in range(3) if lo[a] != full[0][a]]
        moved += [f"{'xyz'[a]}max" for a in range(3) if hi[a] != full[1][a]]
        assert found and moved == [name]
    flat = [ac.flat_index(ac.FACES_SHAPE, at) for at in ac.FACES.values()]
    assert len({(i % ac.BOX_ROUND) // ac.RED_BLOCK for i in flat}) == 6        # six blocks
    assert len({i % 64 for i in flat}) == 6                                      # six lanes
    assert sum(i >= ac.BOX_ROUND for i in flat) == 1                             # one in the second round


def test_the_fused_case_is_found_in_both_tiles_and_line_groups():
    seg = ar.segment(ac.fused_image(), ac.FUSED_BACKGROUND, ac.FUSED_RADIUS)
    assert seg["found"] and (seg["bounds_min"], seg["bounds_max"]) == ac.FUSED_BOX
    assert ac.tile_of(ac.FUSED_RADIUS) == ac.TILE_LARGE
    assert seg["bounds_min"][2] < ac.TILE_LARGE <= seg["bounds_max"][2] < ac.FUSED_SHAPE[0]
    assert seg["bounds_min"][0] < ac.LINES <= seg["bounds_max"][0] < ac.FUSED_SHAPE[2]


@pytest.mark.parametrize("r", list(ac.EXACT))
def test_the_exact_threshold_case_sits_on_the_threshold(r):
    img = ac.exact_image(r)
    seg = ar.segment(img, ac.EXACT_BACKGROUND, r)
    assert (seg["min"], seg["max"], seg["threshold"]) == (0.0, 1.0, 0.5)
    values, counts = np.unique(seg["filtered"], return_counts=True)
    assert values.tolist() == [0.0, 0.5, float(ac.ABOVE)] and counts[1] > counts[2] > 0
    assert (seg["bounds_min"], seg["bounds_max"], seg["found"]) == (*ac.EXACT[r][3], True)
    with np.errstate(invalid="ignore"):          # v >= threshold takes the region of 0.5 in
        idx = np.nonzero(seg["filtered"].astype(np.float64) >= seg["threshold"])
    assert [int(idx[2 - a].min()) for a in range(3)] != seg["bounds_min"]


def test_the_nan_case_tells_the_comparisons_apart():
    clean, dirty = ac.nan_images()
    thr = ar.segment(clean, ac.NAN_BACKGROUND, ac.NAN_RADIUS)["threshold"]
    filt = ar.min_filter(dirty, ac.NAN_RADIUS)
    want = ar.threshold_bounds(filt, thr)
    assert want == (*ac.NAN_BOX, True) and np.isnan(filt).sum() == 5 ** 3
    lo, hi, _ = ac.bounds_not_below(filt, thr)          # the footprint: beyond the box in x and y
    assert lo[0] < want[0][0] and hi[1] > want[1][1] and (lo, hi) != want[:2]
    seg = ar.segment(dirty, ac.NAN_BACKGROUND, ac.NAN_RADIUS)
    assert np.isnan(seg["threshold"]) and not seg["found"]
    assert (seg["bounds_min"], seg["bounds_max"]) == (list(ac.NAN_SHAPE[::-1]), [0, 0, 0])
    assert ac.bounds_not_below(seg["filtered"], seg["threshold"])[:2] == (
        [0, 0, 0], [n - 1 for n in ac.NAN_SHAPE[::-1]])


# ------------------------------------------------------------------ min / max
def test_min_max_fast_is_the_literal_loop():
    """on the small lengths with every plant, and on the special images"""
    for n in (n for n in ac.MINMAX_LENGTHS if n <= 257):
        images = [ac.planted(n, at, v) for at in ac.plant_indices(n) for v in (-1.0, 2.0)]
        images += list(ac.minmax_specials(n).values())
        for img in images:
            np.testing.assert_array_equal(u32(ar.min_max_fast(img)), u32(ar.min_max(img)))
    sp = ac.minmax_specials(65)
    assert all(np.isnan(v) for v in ar.min_max(sp["nan_last"]))
    assert u32(ar.min_max(sp["negative_zero_last"])).tolist() == [0x80000000, 0]
    assert u32(ar.min_max(sp["positive_zero_last"])).tolist() == [0x80000000, 0]
    assert ar.min_max(sp["all_pinf"]) == (ar.FLOAT_MAX, np.inf)
    assert ar.min_max(sp["all_ninf"]) == (-np.inf, -ar.FLOAT_MAX)


def test_min_max_cases_place_the_extrema_where_they_can_be_missed():
    assert ac.ROUND == 262144 and ac.MINMAX_LENGTHS[-1] == 2 * ac.ROUND + 257
    n = ac.MINMAX_LENGTHS[-1]
    at = ac.plant_indices(n)
    assert at == [0, 63, 64, 255, 256, ac.ROUND - 1, ac.ROUND, n - 1]
    # a wave's last lane, a block's last thread, the last element of the first round, the first
    # of the second, and the tail: the third round's second block, one thread of it
    assert (n - 1) // ac.ROUND == 2 and ((n - 1) % ac.ROUND) // ac.RED_BLOCK == 1 and (n - 1) % ac.RED_BLOCK == 0
    for m in ac.MINMAX_LENGTHS:
        for shape in ac.minmax_shapes(m):
            assert int(np.prod(shape)) == m
    assert ac.minmax_shapes(257) == [(1, 1, 257)] and len(ac.minmax_shapes(n)) == 2
    assert ac.plant_indices(1) == [0] and ac.plant_indices(64) == [0, 63]
