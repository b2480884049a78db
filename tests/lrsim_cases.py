"""Case table shared by tests/test_gpu_lrsim_edges.py (csrc/lrsim.hip at its edges) and
tests/test_lrsim_premises_cpu.py (the properties of these cases that the GPU tests rely
on, proved without a GPU).

Conventions: volumes and kernels are float32 [z, y, x] arrays; shapes and kernel sizes
are (z, y, x) here.  The launch arithmetic below restates csrc/lrsim.hip and csrc/fft.cpp.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from oracle import lrsim_ref as ref
from oracle.mvdecon_ref import convolve

MIN32 = np.float32(ref.MIN_VALUE)

# ------------------------------------------------------------------ launch arithmetic
BLOCK, WAVES = 256, 4            # kB, kW of csrc/lrsim.hip
MAX_BLOCKS = 4096                # grid_of's cap for the voxel and the row kernels
VOXELS_PER_SWEEP = MAX_BLOCKS * BLOCK    # 1,048,576: beyond, a voxel kernel loops
ROWS_PER_SWEEP = MAX_BLOCKS * WAVES      # 16,384: beyond, a row kernel loops
REDUCE_THREADS = 1024            # k_lr_sum2 and k_reduce_partials: beyond, they loop


def smooth2357(m: int) -> bool:
    for p in (2, 3, 5, 7):
        while m % p == 0:
            m //= p
    return m == 1


def fft_fast_size(need: int, even: bool) -> int:
    """csrc/fft.cpp: the smallest m >= need of the form 2^a 3^b 5^c 7^d (even when ``even``)."""
    m = max(1, int(need))
    while (even and m % 2) or not smooth2357(m):
        m += 1
    return m


def reach(ksizes):
    """(cz, cy, cx): the largest kernel half-width over the views, per axis."""
    return tuple(max(k[d] // 2 for k in ksizes) for d in range(3))


def padded(shape, ksizes):
    """(Mz, My, Mx) of lrsim_init: fft_fast_size(n + 2 c), even in x."""
    c = reach(ksizes)
    return tuple(fft_fast_size(shape[d] + 2 * c[d], d == 2) for d in range(3))


def ncplx(shape, ksizes) -> int:
    """Hx * My * Mz, the complex count of the R2C spectrum."""
    mz, my, mx = padded(shape, ksizes)
    return (mx // 2 + 1) * my * mz


def blocks(work: int, per_block: int) -> int:
    """grid_of(work, per_block, 4096)."""
    return max(1, min(-(-work // per_block), MAX_BLOCKS))


def voxel_trips(n: int) -> int:
    """Trips of the busiest thread's grid-stride loop in a voxel kernel."""
    return -(-n // (blocks(n, BLOCK) * BLOCK))


def row_trips(rows: int) -> int:
    return -(-rows // (blocks(rows, WAVES) * WAVES))


def mirror_folds(c: int, n: int) -> int:
    """How often the furthest padded position, -c, is reflected back into [0, n)."""
    return 0 if n == 1 else -(-c // (n - 1))


# the volumes of tests/test_gpu_lrsim.py with their kernels: none has an odd ncplx
_SIZES = [(11, 9, 7), (5, 7, 9), (9, 5, 5)]
EXISTING = [((40, 36, 44), _SIZES), ((24, 28, 20), _SIZES), ((1, 30, 26), [(1, 7, 5)] * 3),
            ((28, 24, 30), _SIZES), ((8, 8, 8), [(3, 3, 3)])]


# ------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    shape: tuple                 # (z, y, x)
    ksizes: tuple                # per view (kz, ky, kx)
    weights: str = "positive"    # recipe, see _weights
    image: str = "random"        # or "zero_block"
    iters: int = 2
    rules: tuple = ((False, 0.0), (True, 0.006))   # (multiplicative, lambda)
    seed: int = 0


K3 = (3, 3, 3)
ALL_RULES = ((False, 0.0), (True, 0.0), (False, 0.006), (True, 0.006))
CASES = {
    # Hx, My, Mz all odd: 12 x 9 x 5 -> ncplx = 7 * 9 * 5 = 315, no slack
    "odd_tail": Case((3, 7, 10), (K3, K3), seed=1),
    # only Hx even, My and Mz odd, slack in x (13 -> 14)
    "odd_tail_even_hx": Case((3, 7, 11), (K3, K3), seed=2),
    # ncplx odd with slack: z 24 + 2 -> 27
    "odd_tail_slack": Case((24, 7, 10), (K3, K3), seed=3),
    "odd_dims": Case((13, 17, 21), ((3, 5, 7), (7, 3, 5), (5, 7, 3)), weights="sparse", iters=3, seed=4),
    "many_voxels": Case((6, 420, 420), (K3, K3), weights="sparse", iters=1, rules=ALL_RULES, seed=5),
    "many_rows": Case((130, 130, 6), (K3, K3), iters=1, seed=6),
    "long_reach_x2": Case((5, 6, 2), ((3, 3, 7), K3), seed=7),
    "long_reach_x3": Case((5, 6, 3), ((3, 3, 9), K3), seed=8),
    "long_reach_y2": Case((5, 2, 6), ((3, 7, 3), K3), seed=9),
    "long_reach_y3": Case((5, 3, 6), ((3, 9, 3), K3), seed=10),
    "long_reach_z2": Case((2, 5, 6), ((7, 3, 3), K3), seed=11),
    "long_reach_z3": Case((3, 5, 6), ((9, 3, 3), K3), seed=12),
    # one iteration: after it psi = minValue on the rows without a positive weight, a second one
    # divides the images there by 1e-4, and with quotients of 1e4 beside quotients of 1 a float
    # transform's error floor (1e-7 of the largest value) is 2e-4 of psi -- in the oracle with
    # float32 convolutions as well (test_float_transforms_resolve_every_case)
    "weights": Case((9, 12, 14), ((3, 3, 5), (3, 5, 3), (5, 3, 3)), weights="regions", iters=1, rules=ALL_RULES,
                    seed=13),
    "no_overlap": Case((6, 7, 9), (K3, (3, 5, 3)), weights="disjoint", seed=14),
    "delta": Case((5, 7, 9), ((1, 1, 1),) * 3, weights="sparse", iters=1, rules=ALL_RULES[:2], seed=15),
    "clamp": Case((8, 9, 10), (K3, K3), image="zero_block", rules=ALL_RULES, seed=16),
}
LONG_REACH = {"long_reach_x2": 2, "long_reach_x3": 2, "long_reach_y2": 1, "long_reach_y3": 1,
              "long_reach_z2": 0, "long_reach_z3": 0}   # case -> the axis under test

# y slabs of the "regions" weights (12 rows):
#   [0, 2)  every view exactly 0            -> no view counts, none positive
#   [2, 4)  every view negative             -> all count for the overlap (!= 0), none positive
#   [4, 6)  view 0 positive, the others 0   -> seen by one view only
#   [6, 8)  view 0 positive, view 1 negative, view 2 zero: two views count, one is positive
#   [8, 12) every view positive
REGION_ROWS = {"zero": (0, 2), "negative": (2, 4), "single": (4, 6), "mixed": (6, 8), "all": (8, 12)}
# the zero block of the "zero_block" images: 5 wide on every axis (reach 1), touching y = 0
ZERO_BLOCK = (slice(2, 7), slice(0, 5), slice(4, 9))


def rows(name):
    a, b = REGION_ROWS[name]
    return (slice(None), slice(a, b), slice(None))


def _weights(recipe, shape, nviews, rng):
    ws = [(rng.random(shape) * 0.95 + 0.05).astype(np.float32) for _ in range(nviews)]
    if recipe == "positive":
        return ws
    if recipe == "sparse":      # a fifth of the voxels of every view is exactly 0
        return [w * (rng.random(shape) > 0.2) for w in ws]
    if recipe == "regions":
        for v, w in enumerate(ws):
            w[rows("zero")] = 0.0
            w[rows("negative")] *= -1.0
            if v > 0:
                w[rows("single")] = 0.0
            if v == 1:
                w[rows("mixed")] *= -1.0
            if v == 2:
                w[rows("mixed")] = 0.0
        return ws
    if recipe == "disjoint":    # view v in its own x range, one column between them seen by none
        assert nviews == 2
        cut = shape[2] // 2
        ws[0][:, :, cut:] = 0.0
        ws[1][:, :, :cut + 1] = 0.0
        return ws
    raise ValueError(recipe)


@functools.lru_cache(maxsize=None)
def build(name):
    """(imgs, weights, kernels) of a case: deterministic, read-only."""
    c = CASES[name]
    rng = np.random.default_rng(7700 + c.seed)
    nv = len(c.ksizes)
    imgs = [(rng.random(c.shape) + 0.5).astype(np.float32) for _ in range(nv)]
    if c.image == "zero_block":
        for i in imgs:
            i[ZERO_BLOCK] = 0.0
    ws = _weights(c.weights, c.shape, nv, rng)
    # un-normalised, no small taps: a voxel that sees any non-zero quotient stays far above minValue
    ks = [((rng.random(k) + 0.5) * 3.0).astype(np.float32) for k in c.ksizes]
    out = tuple(tuple(np.ascontiguousarray(a, np.float32) for a in g) for g in (imgs, ws, ks))
    for g in out:
        for a in g:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, mult, lam, views_of=None):
    """(psi, avg, stats) of oracle/lrsim_ref.py for one rule of a case (read-only)."""
    imgs, ws, ks = build(name)
    vo = None if views_of is None else [list(v) for v in views_of]
    psi, avg, st = ref.lucy_richardson_multi_view(list(imgs), list(ws), list(ks), CASES[name].iters, mult, lam,
                                                  views_of=vo)
    psi.setflags(write=False)
    return psi, avg, tuple(st)


def oracle_at_precision(name, mult, lam, precision):
    """The oracle's iteration (lrsim_ref.lucy_richardson_multi_view) with the convolutions
    at ``precision`` ('f64', as the oracle, or 'f32': single-precision FFTs)."""
    imgs, ws, ks = build(name)
    ks = [ref.norm_image(k) for k in ks]
    psi = np.full(CASES[name].shape, np.float32(ref.norm_all_images(imgs, ws)), np.float32)
    for _ in range(max(1, CASES[name].iters)):
        contribs = []
        for img, k in zip(imgs, ks):
            blurred = convolve(psi, k, "mirror", precision=precision)
            with np.errstate(all="ignore"):
                q = (img / blurred).astype(np.float32)
            contribs.append(convolve(q, k, "mirror", precision=precision))
        nxt = ref.combine(psi, contribs, ws, mult)
        if lam > 0:
            nxt = ref.tikhonov(nxt, lam)
        psi, _, _ = ref.finish(psi, nxt)
    return psi


def delta_closed_form(imgs, ws, avg, mult):
    """One iteration from psi = avg with 1x1x1 kernels: the weighted arithmetic (geometric)
    mean of the views' img / psi, times psi; minValue where no view is positive."""
    p0 = np.float32(avg)
    w = np.stack(ws).astype(np.float64)
    q = np.stack([(i / p0).astype(np.float32) for i in imgs]).astype(np.float64)
    m = w > 0
    num = np.where(m, w, 0).sum(0)
    safe = np.where(num > 0, num, 1)
    if mult:
        val = np.exp(np.where(m, w * np.log(q), 0).sum(0) / safe)
    else:
        val = np.where(m, q * w, 0).sum(0) / safe
    out = np.where(num > 0, np.float64(p0) * val, ref.MIN_VALUE)
    return np.maximum(ref.MIN_VALUE, out.astype(np.float32)).astype(np.float32)


def positive_count(ws):
    return sum((w > 0).astype(np.int64) for w in ws)


def nonzero_count(ws):
    return sum((w != 0).astype(np.int64) for w in ws)


# ------------------------------------------------------------------ the rule, voxel by voxel
RULE_N = (1 << 20) + 77          # one full sweep of k_lr_update's 4096 blocks and a ragged tail
RULE_LAMBDAS = (0.0, 0.006, 0.3, 1e-7)
NUM_SPECIAL = [0.0, -0.0, 5e-324, 1e-300]
VALUE_SPECIAL = [0.0, -0.0, -1.75, np.nan, np.inf, -np.inf, 5e-324, 1e300]
PSI_SPECIAL = [1e-4, 0.0, 3e38]


@functools.lru_cache(maxsize=None)
def rule_inputs(specials: bool):
    """(psi float32, value float64, num float64) over RULE_N voxels: random magnitudes over
    many binades, a share of negative values, and (``specials``) every combination of the
    special psi / value / num with each other and with ordinary operands, the last of them
    in the ragged tail."""
    rng = np.random.default_rng(991)
    n = RULE_N
    psi = (rng.random(n) * 10).astype(np.float32)
    value = 2.0 ** rng.uniform(-30, 30, n)
    value[: n // 8] = rng.standard_normal(n // 8) * 3
    num = rng.random(n) * 3 + 0.25     # pow(value, 1 / num) stays finite in float
    if specials:
        ps = [np.float32(p) for p in PSI_SPECIAL] + [np.float32(2.5)]
        vs = VALUE_SPECIAL + [0.8, 37.0]
        ns = NUM_SPECIAL + [1.0, 0.37]
        combos = [(p, v, m) for p in ps for v in vs for m in ns]
        for start in (n // 4, n - len(combos)):      # the second copy ends at the last voxel
            for j, (p, v, m) in enumerate(combos):
                psi[start + j], value[start + j], num[start + j] = p, v, m
    for a in (psi, value, num):
        a.setflags(write=False)
    return psi, value, num


def rule_oracle(psi, value, num, mult, lam):
    """apply_value + tikhonov + finish of oracle/lrsim_ref.py: (new psi, sum, max |change|)."""
    nxt = ref.apply_value(psi, value, num, mult)
    if lam > 0:
        nxt = ref.tikhonov(nxt, lam)
    return ref.finish(psi, nxt)
