"""The cases of tests/resample_cases.py have the properties that
tests/test_gpu_resample_edges.py relies on -- proved on the oracle alone, no GPU."""
import numpy as np
import pytest

import resample_cases as rc
from oracle import input_ref as ir

TIE_CAP = 1e-3   # the cap of assert_mismatches_on_ties on the share of excused voxels


def _tie_cases():
    """Every (models, bb_min, bb_dims, ds, half) that goes through the ties helper."""
    out = {}
    _, m, b0, bd = rc.crop_case()
    out["crop"] = (m, b0, bd, 1.0, False)
    _, m, b0, bd = rc.stride_case()
    out["stride sub-box"] = (m, rc.sub_box(b0, rc.STRIDE_SUB_OFF), rc.STRIDE_SUB_DIMS, 1.0, False)
    for d in rc.DEGENERATE_DIMS:
        _, m, b0, bd = rc.degenerate_case(d)
        out[f"degenerate {d}"] = (m, b0, bd, 1.0, False)
        out[f"degenerate {d} nearest"] = (m, b0, bd, 1.0, True)
    m, b0, bd = rc.ramp_models()["large"]
    out["large"] = ([m], b0, bd, 1.0, False)
    out["large downsampled nearest"] = ([m], b0, rc.large_ds_dims(bd), rc.LARGE_DS, True)
    for V in (1, 7):
        _, m, b0, bd = rc.count_case(V)
        out[f"V={V}"] = (m, b0, bd, 1.0, False)
        out[f"V={V} nearest"] = (m, b0, bd, 1.0, True)
    _, m, b0, bd = rc.base_case()
    out["base"] = (m, b0, bd, 1.0, False)
    return out


@pytest.mark.parametrize("name", sorted(_tie_cases()))
def test_p1_ties_are_rare(name):
    """P1: far fewer voxels sit on a float32 position tie than the helper's cap lets
    through, so the cap can never hide a real failure."""
    models, b0, bd, ds, half = _tie_cases()[name]
    assert rc.tie_share(models, b0, bd, ds, half) < TIE_CAP


def test_crop_boxes_lie_inside_and_see_data():
    srcs, models, b0, bd = rc.crop_case()
    imgs = [ir.transform_view(s, m, b0, bd, rc.BORDER, rc.RANGE, ir.NO_WEIGHTS)[0] for s, m in zip(srcs, models)]
    for off, dims in rc.CROP_BOXES:
        assert all(o >= 0 and o + d <= b for o, d, b in zip(off, dims, bd)), (off, dims)
        assert any((rc.crop(i, off, dims) > 0).any() for i in imgs), (off, dims)
    tx, tz = 32, 8   # kTileX, kTileZ of csrc/resample.hpp
    dims = [d for _, d in rc.CROP_BOXES]
    assert any(d[0] < tx and d[2] < tz for d in dims) and any(d[0] == tx and d[2] == tz for d in dims)
    assert any(d[0] == tx + 1 and d[2] == tz + 1 for d in dims) and any(d[1] == 1 for d in dims)


@pytest.mark.parametrize("wt", [ir.PRECOMPUTED_WEIGHTS, ir.VIRTUAL_WEIGHTS])
@pytest.mark.parametrize("T", rc.STATS_THREADS)
def test_p2_portions_unequal_and_mean_of_means_differs(T, wt):
    """P2: the last portion is longer and sees fewer views, so the reference's mean of
    per-portion means (WeightNormalizer.java:74-86) is not the global mean; an
    implementation that averaged over the box would miss avg_overlap."""
    raw = rc.raw_weights("stats", wt)
    n = raw[0].size
    lengths = rc.portion_lengths(n, T)
    assert n % (2 * T) != 0 and lengths[-1] > lengths[0] and sum(lengths) == n
    count = sum((w > 0).astype(np.int64) for w in raw)
    _, _, mn, av = ir.normalize_weights(list(raw), wt, T)
    assert abs(av - count.mean()) > 1e-6
    # a last portion of n // 2T voxels (dropping the remainder) gives another mean as well
    flat = count.reshape(-1)
    assert flat[-lengths[-1]:].any()
    short = [flat[q * lengths[0]:(q + 1) * lengths[0]].mean() for q in range(2 * T)]
    assert abs(av - float(np.mean(short))) > 1e-6
    assert av > 1.0 and mn == 0 and (flat == len(raw)).any()   # osem_index 2 is not clamped to 1


def test_tiny_box_has_fewer_voxels_than_portions():
    raw = rc.raw_weights("tiny", ir.VIRTUAL_WEIGHTS)
    assert raw[0].size == 12 < 2 * 8
    _, _, mn, av = ir.normalize_weights(list(raw), ir.VIRTUAL_WEIGHTS, 8)
    assert np.isnan(av) and mn == 2
    assert ir.osem_speedup(2, 1.0, mn, av) == 1.0   # max(1.0, NaN) here; Java's Math.max gives NaN


@pytest.mark.parametrize("dims", rc.DEGENERATE_DIMS)
def test_p3_degenerate_cases_fill_the_mirrored_band(dims):
    """P3: at least 5 % of the voxels inside each view lie in t_d in (s_d - 1, s_d) on
    some axis, where the upper corner mirrors to s_d - 2 (to 0 for s_d = 1)."""
    srcs, models, b0, bd = rc.degenerate_case(dims)
    for s, m in zip(srcs, models):
        share, inside = rc.band_share(s, m, b0, bd)
        assert inside >= 1000 and share >= 0.05
    if 1 in dims:   # the 1-thick source: every inside voxel has t_z in [0, 1)
        assert all(rc.band_share(s, m, b0, bd)[0] == 1.0 for s, m in zip(srcs, models))


def test_p4_seven_views_cover_the_box_unevenly():
    """P4: PRECOMPUTED weights are NaN where no view has a weight; the V = 7 box has
    such voxels, and voxels under 1, under 2..6 and under all 7 views."""
    raw = rc.raw_weights("count7", ir.PRECOMPUTED_WEIGHTS)
    count = sum((w > 0).astype(np.int64) for w in raw)
    hist = np.bincount(count.reshape(-1), minlength=8)
    assert 0 < hist[0] < count.size
    assert hist[1] > 0 and hist[2:7].sum() > 0 and hist[7] > 0
    ws, _, _, _ = ir.normalize_weights(list(raw), ir.PRECOMPUTED_WEIGHTS, 8)
    assert np.array_equal(np.isnan(ws[0]), count == 0)


@pytest.mark.parametrize("T", rc.STRIDE_THREADS)
def test_p5_weight_sum_strides(T):
    """P5: with the launch geometry of csrc/input_prep.hip:323-324 the largest portion is
    longer than one sweep of the capped x grid, so threads take a second voxel."""
    n = int(np.prod(rc.STRIDE_BB_DIMS))
    nportions, span, bx = rc.weight_sum_launch(n, T)
    cap = rc.K_WEIGHT_SUM_MAX_BLOCKS // nportions
    assert n > rc.K_WEIGHT_SUM_MAX_BLOCKS * rc.K_WEIGHT_SUM_BLOCK
    assert bx == cap and span > cap * rc.K_WEIGHT_SUM_BLOCK
    assert n % nportions != 0
    raw = rc.raw_weights("stride", ir.VIRTUAL_WEIGHTS)
    count = sum((w > 0).astype(np.int64) for w in raw)
    assert all((count == c).mean() > 0.05 for c in (0, 1, 2))   # both views partly cover the box


@pytest.mark.parametrize("name", sorted(rc.ramp_models()))
def test_p6_ramp_boxes_and_models(name):
    """P6: each ramp box has at least 30 % of its voxels strictly inside the source and
    10 % strictly outside; the shear and reflection inverses are far from their
    transposes, so a transposed inverse moves positions by whole voxels."""
    m, b0, bd = rc.ramp_models()[name]
    _, inside, outside, t = rc.ramp_reference(m, b0, bd)
    assert inside.mean() >= 0.30 and outside.mean() >= 0.10
    assert not (inside & outside).any()
    inv = np.linalg.inv(m[:, :3])
    if name in ("shear", "reflection"):
        assert np.abs(inv - inv.T).max() > 0.1
        wrong = t[inside] @ (inv.T @ m[:, :3]).T   # inv^T (p - tr) instead of inv (p - tr)
        assert np.abs(wrong - t[inside]).max() > 1.0
    if name == "reflection":
        assert np.linalg.det(m[:, :3]) < 0
    if name == "large":
        assert min(abs(v) for v in b0) > 1500 and np.abs(m[:, 3]).min() > 1500
    z = m[:, :3] @ np.array([0.0, 0.0, 1.0])
    if name != "shear":
        assert 1.6 <= np.linalg.norm(z) <= 3.2
    assert max(rc.RAMP_DIMS) <= 48 and all(4 * v == int(4 * v) for v in rc.RAMP_SLOPE + (rc.RAMP_D,))
    assert rc.ramp_source().min() > 1.0   # max(minValue, f) is f
