"""Case builders shared by tests/test_gpu_resample_edges.py (the GPU resampling
kernels at their edges) and tests/test_resample_premises_cpu.py (the properties of
these cases that the GPU tests rely on, proved on the oracle alone).

Conventions of the library: sources [z, y, x] float32, models 3x4 (source -> world),
bb_min / bb_dims / source dims (x, y, z).
"""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import input_ref as ir

BORDER, RANGE = (-2, -2, -1), (6, 6, 4)   # blending of the prepare_inputs cases (source pixels)


def rot(axis, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def model(a, t):
    m = np.zeros((3, 4))
    m[:, :3] = a
    m[:, 3] = t
    return m


def random_source(dims_xyz, seed):
    """Positive float32 noise, [z, y, x]."""
    sx, sy, sz = dims_xyz
    return (np.random.default_rng(seed).random((sz, sy, sx)) * 100 + 1).astype(np.float32)


def fan_views(V, dims_xyz=(22, 20, 18), seed=5, step=None, about_centre=False):
    """V anisotropic views rotated about y by ``step`` degrees apart (360 / V by
    default; the family of test_gpu_input_prep.views, sources 18x20x22 as [z, y, x]).
    The rotations turn about the source's origin corner or, with ``about_centre``,
    about its centre, so that every view covers the neighbourhood of that point."""
    srcs, models = [], []
    step = 360.0 / V if step is None else step
    for v in range(V):
        srcs.append(random_source(dims_xyz, seed + v))
        a = rot("y", step * v + 7) @ rot("z", 5 * v) @ np.diag([1.0, 1.0, 1.6])
        t = np.array([2.3 + v, -1.7, 3.1 * v])
        if about_centre:
            t = t - a @ ((np.array(dims_xyz) - 1) / 2.0)
        models.append(model(a, t))
    return srcs, models


def sub_box(bb_min, off):
    return tuple(int(b) + int(o) for b, o in zip(bb_min, off))


def crop(vol, off, dims):
    """The [z, y, x] slice of an enclosing-box volume that a sub-box at offset off covers."""
    return vol[off[2]:off[2] + dims[2], off[1]:off[1] + dims[1], off[0]:off[0] + dims[0]]


# ------------------------------------------------------------------ 1. crop invariance
CROP_BB_MIN, CROP_BB_DIMS = (-34, -22, -10), (76, 44, 24)
# (offset inside the enclosing box, dims): narrower than a 32 x 8 (x, z) tile, exactly one
# tile, one voxel past a tile in x and z, two tiles each way with ny = 1, a tall thin
# box, and nz = 1 over three x tiles
CROP_BOXES = [((38, 34, 14), (1, 1, 1)), ((20, 17, 6), (31, 5, 7)), ((19, 18, 5), (32, 4, 8)),
              ((18, 19, 4), (33, 3, 9)), ((7, 21, 3), (64, 1, 16)), ((33, 2, 11), (5, 40, 3)),
              ((3, 20, 13), (70, 2, 1))]
CROP_FUSE_BOXES = [CROP_BOXES[3], CROP_BOXES[5]]
CROP_FUSE_BORDERS, CROP_FUSE_RANGES = [(0, 0, 0), (1, 1, 0), (-1, 0, -1)], [(5, 5, 3), (4, 6, 3), (6, 4, 5)]


def crop_case():
    srcs, models = fan_views(3)
    return srcs, models, CROP_BB_MIN, CROP_BB_DIMS


# ------------------------------------------------------------------ 2. overlap statistics
# n = 37 * 31 * 29 = 33263: odd and 2 mod 3, so n mod 2T != 0 for T = 1, 3, 8; the views
# thin out towards the box's last z planes, so the last portion (which takes the
# remainder) sees fewer views than the others, but not none
STATS_BB_MIN, STATS_BB_DIMS = (0, -4, 5), (37, 31, 29)
STATS_THREADS = (1, 3, 8)
TINY_BB_MIN, TINY_BB_DIMS = (3, 2, 4), (3, 2, 2)   # n = 12 < 2 * 8 portions


def stats_case():
    srcs, models = fan_views(3, step=9.0)
    return srcs, models, STATS_BB_MIN, STATS_BB_DIMS


def portion_lengths(n, ij_threads):
    return [loop for _, loop in ir.divide_into_portions(n, 2 * ij_threads)]


@functools.lru_cache(maxsize=None)
def raw_weights(case, weight_type):
    """The oracle's per-view blending weights before normalisation, from the positions
    alone (no interpolation): cheap enough for the 2.2-Mvoxel box."""
    srcs, models, bb_min, bb_dims = CASES[case]()
    out = []
    for s, m in zip(srcs, models):
        dims = (s.shape[2], s.shape[1], s.shape[0])
        t = (ir.image_positions(m, bb_min, bb_dims) if weight_type == ir.PRECOMPUTED_WEIGHTS
             else ir.weight_positions(m, bb_min, bb_dims))
        w = ir.blending_weight(t, dims, BORDER, RANGE)
        w.setflags(write=False)
        out.append(w)
    return tuple(out)


def expected_weights(case, weight_type, ij_threads, osem_index=0, osem=1.0):
    """(final weights, min_overlap, avg_overlap, osem used) of the oracle."""
    ws, S, mn, av = ir.normalize_weights(list(raw_weights(case, weight_type)), weight_type, ij_threads)
    o = ir.osem_speedup(osem_index, osem, mn, av)
    return ir.final_weights(ws, S, weight_type, o), mn, av, o


# ------------------------------------------------------------------ 3. grid-stride path
# n = 137 * 129 * 127 = 2,244,471 > 8192 * 256: each thread of k_weight_sum strides over
# more than one voxel; odd, so the portions are unequal as well
STRIDE_BB_MIN, STRIDE_BB_DIMS = (-8, -6, -5), (137, 129, 127)
STRIDE_THREADS = (8, 64)
STRIDE_SUB_OFF, STRIDE_SUB_DIMS = (60, 50, 30), (40, 40, 40)
K_WEIGHT_SUM_BLOCK, K_WEIGHT_SUM_MAX_BLOCKS = 256, 8192


def weight_sum_launch(n, ij_threads):
    """(portions, largest portion, x blocks) of k_weight_sum's launch, by the formula of
    spim_registration_amd/csrc/input_prep.hip:323-324."""
    nportions = 2 * ij_threads
    span = max(n // nportions, n - (n // nportions) * (nportions - 1))
    bx = max(1, min(-(-span // K_WEIGHT_SUM_BLOCK), K_WEIGHT_SUM_MAX_BLOCKS // nportions))
    return nportions, span, bx


def stride_case():
    """Two 24^3 sources magnified about five times: each covers part of the box."""
    srcs = [random_source((24, 24, 24), 31), random_source((24, 23, 22), 32)]
    models = [model(rot("y", 11) @ rot("z", 7) @ np.diag([4.6, 4.9, 5.3]), [3.3, -2.6, 1.2]),
              model(rot("x", -9) @ rot("y", -17) @ np.diag([5.2, 4.4, 4.8]), [41.7, 22.4, 8.9])]
    return srcs, models, STRIDE_BB_MIN, STRIDE_BB_DIMS


# ------------------------------------------------------------------ 4. degenerate sources
DEGENERATE_DIMS = [(13, 9, 1), (2, 9, 7), (2, 2, 2)]
DEGENERATE_FUSE_BORDERS, DEGENERATE_FUSE_RANGES = [(-1, -1, -1), (0, -1, -2)], [(3, 3, 2), (2, 4, 3)]


def degenerate_case(dims_xyz):
    """Two views of a 1- or 2-thick source, one rotated and one axis-aligned, with
    fractional translations and a z scale; the thin axes are magnified so that many
    output voxels fall between the last plane and the source's end."""
    sx, sy, sz = dims_xyz
    scale = [6.53 if sx <= 2 else 1.31, 5.47 if sy <= 2 else 1.23, 7.12 if sz <= 2 else 2.43]
    srcs = [random_source(dims_xyz, 41), random_source(dims_xyz, 42)]
    models = [model(rot("z", 13) @ rot("x", 9) @ np.diag(scale), [1.37, -0.62, 0.81]),
              model(np.diag(scale) * [1.0, 1.07, 0.93], [-2.47, 1.73, -1.29])]
    ext = np.array(scale) * np.array(dims_xyz)
    bb_min = tuple(int(v) for v in np.floor(-0.35 * ext - 3))
    bb_dims = tuple(int(v) for v in np.ceil(1.6 * ext + 8))
    return srcs, models, bb_min, bb_dims


# ------------------------------------------------------------------ 5. analytic ramp
RAMP_DIMS = (40, 36, 28)                     # (x, y, z), at most 48 per axis
RAMP_SLOPE, RAMP_D = (0.75, -1.25, 2.5), 60.0   # multiples of 1/4; f >= 11.25 > minValue
RAMP_MARGIN = 1e-3


def ramp(t):
    """f at positions t[..., 3] (x, y, z), float64."""
    return RAMP_SLOPE[0] * t[..., 0] + RAMP_SLOPE[1] * t[..., 1] + RAMP_SLOPE[2] * t[..., 2] + RAMP_D


def ramp_source():
    sx, sy, sz = RAMP_DIMS
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    f = ramp(np.stack([x, y, z], -1).astype(np.float64))
    src = f.astype(np.float32)
    assert np.array_equal(src.astype(np.float64), f)   # exactly representable
    return src


def _ramp_box(m, bb_dims):
    """bb_min that centres the box on the image of the source's centre."""
    c = m[:, :3] @ ((np.array(RAMP_DIMS) - 1) / 2.0) + m[:, 3]
    return tuple(int(v) for v in np.round(c - np.array(bb_dims) / 2.0))


def ramp_models():
    """name -> (model, bb_min, bb_dims)."""
    out = {}
    a = rot("y", 24) @ rot("z", 11) @ np.diag([1.0, 1.0, 2.4])
    out["rotation"] = model(a, [3.3, -4.6, 2.2])
    out["shear"] = model(np.array([[1.0, 0.45, 0.3], [0.0, 1.0, 0.55], [0.0, 0.0, 1.6]]), [-5.25, 1.4, 0.7])
    out["reflection"] = model(rot("z", 17) @ rot("x", -8) @ np.diag([-1.0, 1.0, 3.0]), [21.3, 2.9, -6.1])
    out["large"] = model(rot("y", -19) @ rot("x", 14) @ np.diag([1.0, 1.0, 1.9]), [4011.37, -2489.58, 1807.91])
    dims = {"rotation": (58, 46, 70), "shear": (62, 50, 48), "reflection": (50, 48, 92), "large": (56, 50, 60)}
    return {k: (m, _ramp_box(m, dims[k]), dims[k]) for k, m in out.items()}


LARGE_DS = 1.5


def large_ds_dims(bb_dims):
    """The box of the large-coordinate model at downsampling LARGE_DS (same extent)."""
    return tuple(int(d / LARGE_DS) for d in bb_dims)


def ramp_reference(m, bb_min, bb_dims, ds=1.0):
    """(f(t64), inside, outside, t64) over the box, independent of oracle/input_ref.py:
    t64 = inv(M) (p - tr) with numpy.linalg.inv in float64.  inside: 0 <= t <= s - 1 on
    every axis by RAMP_MARGIN (n-linear interpolation of f is exact there); outside:
    beyond [0, s) on some axis by the same margin (the kernels write 0 there)."""
    nx, ny, nz = bb_dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = np.stack([x, y, z], -1).astype(np.float64) * ds + np.array(bb_min, np.float64)
    t = (p - m[:, 3]) @ np.linalg.inv(m[:, :3]).T
    s = np.array(RAMP_DIMS, np.float64)
    inside = ((t >= RAMP_MARGIN) & (t <= s - 1 - RAMP_MARGIN)).all(-1)
    outside = ((t < -RAMP_MARGIN) | (t > s + RAMP_MARGIN)).any(-1)
    return ramp(t), inside, outside, t


def ramp_bound(t_inside):
    """16 * 2^-24 * max|f| + sum_d |slope_d| * ulp32(max|t_d|): 8 float roundings of the
    corner products and 7 float adds, each at most 2^-24 * max|f|; the float32 position
    is off by at most one ulp per axis and f moves by |slope_d| times that."""
    fmax = float(np.abs(ramp_source()).max())
    pos = sum(abs(sl) * float(np.spacing(np.float32(np.abs(t_inside[..., d]).max())))
              for d, sl in enumerate(RAMP_SLOPE))
    return 16 * 2.0 ** -24 * fmax + pos


# ------------------------------------------------------------------ 6. view counts
COUNT_BB_MIN, COUNT_BB_DIMS = (-24, -6, -24), (50, 31, 52)
COUNT_FUSE_BORDERS = [(0, 0, 0), (1, 1, 0), (-1, 0, -1), (0, 1, 1), (2, 0, 0), (0, 0, 2), (1, 2, 1)]
COUNT_FUSE_RANGES = [(5, 5, 3), (4, 6, 3), (6, 4, 5), (3, 3, 3), (5, 4, 4), (4, 4, 6), (6, 6, 2)]


def count_case(V):
    srcs, models = fan_views(V, about_centre=True)
    return srcs, models, COUNT_BB_MIN, COUNT_BB_DIMS


# ------------------------------------------------------------------ 7. / 8. the 40x34x30 case
BASE_BB_MIN, BASE_BB_DIMS = (-12, -10, -8), (40, 34, 30)
BASE_FUSE_BORDERS, BASE_FUSE_RANGES = [(0, 0, 0), (1, 1, 0)], [(5, 5, 3), (4, 6, 3)]


def base_case(V=3):
    srcs, models = fan_views(V)
    return srcs, models, BASE_BB_MIN, BASE_BB_DIMS


CASES = {"stats": stats_case, "stride": stride_case, "count7": lambda: count_case(7),
         "count1": lambda: count_case(1),
         "tiny": lambda: fan_views(3) + (TINY_BB_MIN, TINY_BB_DIMS)}


# ------------------------------------------------------------------ premises
def tie_share(models, bb_min, bb_dims, ds=1.0, half=False):
    """Share of box voxels whose float32 source position in some view has a coordinate
    within 4 ulp of an integer (with ``half``, of a half-integer too): the voxels that
    assert_mismatches_on_ties excuses."""
    near = np.zeros((bb_dims[2], bb_dims[1], bb_dims[0]), bool)
    for m in models:
        t = ir.image_positions(m, bb_min, bb_dims, ds)
        t64 = t.astype(np.float64)
        ulp = np.spacing(np.abs(t)).astype(np.float64)
        for off in ((0.0, 0.5) if half else (0.0,)):
            d = np.abs(t64 + off - np.round(t64 + off))
            near |= (d <= 4 * ulp + 1e-12).any(axis=-1)
    return float(near.mean())


def band_share(src, m, bb_min, bb_dims):
    """Among the voxels inside the view, the share whose position lies in the mirrored
    last-plane band t_d in (s_d - 1, s_d) on some axis (for s_d = 1 that is [0, 1))."""
    t = ir.image_positions(m, bb_min, bb_dims).astype(np.float64)
    s = np.array([src.shape[2], src.shape[1], src.shape[0]], np.float64)
    inside = ((t >= 0) & (t < s)).all(-1)
    band = ((t > s - 1) & (t < s)).any(-1) & inside
    return float(band.sum()) / max(1, int(inside.sum())), int(inside.sum())
