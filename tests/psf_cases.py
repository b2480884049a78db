"""Case builders shared by tests/test_gpu_psf_edges.py (csrc/psf.hip at its edges, bit
for bit against oracle/psf_ref.py) and tests/test_psf_premises_cpu.py (the properties
of these cases that the GPU tests rely on, proved on the oracle and NumPy alone).

Conventions of the library: images and PSFs [z, y, x] float32, sizes and bead
locations (x, y, z), models 3x4.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import psf_ref as pr

IMG_DIMS = (12, 10, 8)         # the small periodic image, (x, y, z)
BIG_DIMS = (64, 56, 40)        # the view of the interior class
PSF = (9, 9, 11)
N_MANY, N_FEW = 70, 7          # two-phase path (> 64 beads) and k_psf_extract

ROT = np.array([[0.92, 0.31, 0.05, 140.0], [-0.29, 0.95, 0.12, -33.0], [0.02, -0.15, 2.4, 7.5]])
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def image(dims_xyz=IMG_DIMS, seed=1):
    """normal(0, 1) plus a few spikes: a zero mean keeps the float32 accumulator small, so
    a one-ulp difference of one sample survives the sum over the beads and the
    normalisation."""
    sx, sy, sz = dims_xyz
    rng = np.random.default_rng(seed)
    img = rng.normal(0, 1, (sz, sy, sx)).astype(np.float32)
    for _ in range(5):
        img[rng.integers(sz), rng.integers(sy), rng.integers(sx)] += np.float32(rng.choice([-20.0, 25.0]))
    return img


# ------------------------------------------------------------------ B. bead classes
def _dyadic(rng, lo, hi, n):
    """multiples of 1/16 in [lo, hi) per axis (lo, hi scalars or 3-vectors)"""
    lo, hi = np.broadcast_to(lo, 3), np.broadcast_to(hi, 3)
    return rng.integers(np.round(lo * 16).astype(int), np.round(hi * 16).astype(int), size=(n, 3)) / 16.0


def _large(e, sign):
    def make(rng, n):
        return sign * (2.0 ** e - rng.uniform(0.05, 4.0, (n, 3)))
    return make


def _faces(rng, n):
    """within 5 voxels of a face on every axis, dyadic (exact sums)"""
    s = np.array(IMG_DIMS, float)
    low = _dyadic(rng, 0.0, 5.0, n)
    return np.where(rng.random((n, 3)) < 0.5, low, s - 5.0 + low)


def _last(rng, n):
    """at size - 1 exactly on at least one axis: the upper corner wraps with weight 0"""
    c = _dyadic(rng, 0.0, np.array(IMG_DIMS, float), n)
    on = rng.random((n, 3)) < 0.5
    on[np.arange(n), rng.integers(3, size=n)] = True
    return np.where(on, np.array(IMG_DIMS, float) - 1.0, c)


def _periods(rng, n):
    c = _dyadic(rng, -60.0, 70.0, n)
    c[0], c[1 % n] = (-37.25, 50.5, -37.25), (50.5, -37.25, 50.5)
    return c


def _repeat(rng, n):
    return np.tile(np.array([[5.3, 4.7, 3.2]]), (n, 1))


BEAD_CLASSES = {
    # exact sums, footprint inside (on BIG_DIMS): the fast branch of k_psf_samples
    "interior": lambda rng, n: rng.uniform(8.0, 11.0, (n, 3)),
    # inexact sums at ordinary size: the exactness test sends them to nlinear_at
    "unit": lambda rng, n: rng.uniform(0.0, 1.0, (n, 3)),
    "below_pow2": lambda rng, n: rng.choice([4.0, 8.0, 16.0, 32.0], (n, 3)) - rng.uniform(1e-3, 1.0, (n, 3)),
    # inexact sums that matter in float32
    "large28": _large(28, 1.0), "large29": _large(29, 1.0), "large30": _large(30, 1.0),
    "neglarge30": _large(30, -1.0),
    # exact sums, footprint across the border
    "faces": _faces, "last": _last,
    "integer": lambda rng, n: rng.integers(-3, 15, (n, 3)).astype(np.float64),
    "periods": _periods,
    "negfrac": lambda rng, n: _dyadic(rng, -6.0, 0.0, n) - 1.0 / 32,
    "repeat": _repeat,
}
LARGE_CLASSES = ["large28", "large29", "large30", "neglarge30"]
MIXED_FROM = [k for k in BEAD_CLASSES if k != "repeat"]


def beads(name, n=N_MANY, seed=0):
    """(image, locations [n, 3]) of a bead class; "mixed": every class in turn."""
    key = sorted(BEAD_CLASSES).index(name) if name in BEAD_CLASSES else 99
    rng = np.random.default_rng(1000 * seed + 10 * key + n)
    if name == "mixed":
        per = -(-n // len(MIXED_FROM))
        locs = np.stack([BEAD_CLASSES[k](rng, per) for k in MIXED_FROM], axis=1).reshape(-1, 3)[:n]
    else:
        locs = BEAD_CLASSES[name](rng, n)
    img = image(BIG_DIMS, 2) if name == "interior" else image()
    return img, np.ascontiguousarray(locs, np.float64)


# PSF voxel counts around 256 (one accumulate block) and kPsfSpt * kPsfBlock = 2048 (one
# k_psf_samples block): 255, 256, 257, 2047, 2048, 2049, 2050, 2 * 2048 + 1, and 1 and k x 1 x 1.
# x, y and z each take an even value, an odd value and 1.
SIZES = [(5, 3, 17), (16, 16, 1), (257, 1, 1), (1, 23, 89), (16, 16, 8), (683, 1, 3), (5, 10, 41),
         (17, 241, 1), (1, 1, 1), (7, 1, 1)]


def expected_psf(img, locs, size, chunk=4096):
    """The oracle's normalised original PSF."""
    chunk = max(1, min(chunk, 2 ** 20 // int(np.prod(size))))
    return pr.normalize(pr.extract_psf_local_batched(img, locs, size, chunk=chunk))


def expected(img, locs, size, model=None):
    orig = expected_psf(img, locs, size)
    return orig, (pr.transform_psf(orig, model) if model is not None else None)


# --------------------------------------- the branch of k_psf_samples, restated in NumPy
def _rel(size):
    sx, sy, sz = (int(v) for v in size)
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return np.stack([x - sx // 2, y - sy // 2, z - sz // 2], axis=-1).astype(np.float64)


def branch_masks(img_shape, locs, size):
    """Per (bead, voxel): (every k + c exact by the kernel's test (q - k) == c, footprint
    of floor(c) + k inside the image).  The fast branch runs where both hold."""
    k = _rel(size)[None]
    c = np.asarray(locs, np.float64)[:, None, None, None, :]
    q = k + c
    exact = ((q - k) == c).all(axis=-1)
    b = np.floor(c) + k
    s = np.array([img_shape[2], img_shape[1], img_shape[0]], np.float64)
    inside = ((b >= 0) & (b + 1 < s)).all(axis=-1)
    return exact, inside


def fast_branch_samples(img, locs, size):
    """The fast branch of k_psf_samples forced on every (bead, voxel): the eight weights of
    c - floor(c), base floor(c) + k, periodic gather (so it is defined outside as well),
    FloatType.mul(double) / add in nlinear's corner order.  [n, sz, sy, sx] float32."""
    img = np.asarray(img, np.float32)
    nz, ny, nx = img.shape
    c = np.asarray(locs, np.float64)[:, None, None, None, :]
    f = np.floor(c)
    w = c - f
    wi = 1.0 - w
    b = (f + _rel(size)[None]).astype(np.int64)
    x0, y0, z0 = b[..., 0], b[..., 1], b[..., 2]
    order = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 0, 1), (0, 0, 1)]
    acc = None
    for dx, dy, dz in order:
        wt = (w if dx else wi)[..., 0] * (w if dy else wi)[..., 1] * (w if dz else wi)[..., 2]
        v = img[np.mod(z0 + dz, nz), np.mod(y0 + dy, ny), np.mod(x0 + dx, nx)]
        term = (v.astype(np.float64) * wt).astype(np.float32)
        acc = term if acc is None else (acc + term).astype(np.float32)
    return acc


def oracle_samples(img, locs, size):
    pos = _rel(size)[None] + np.asarray(locs, np.float64)[:, None, None, None, :]
    return pr.nlinear(img, pos, "periodic")


def psf_of_samples(samples):
    """float sum in bead order, normalised"""
    z = np.zeros((1,) + samples.shape[1:], np.float32)
    return pr.normalize(np.add.accumulate(np.concatenate([z, samples]), axis=0, dtype=np.float32)[-1])


def mutant_samples(img, locs, size):
    """k_psf_samples without its exactness test: the fast branch wherever the footprint is
    inside the image, nlinear elsewhere."""
    _, inside = branch_masks(img.shape, locs, size)
    return np.where(inside, fast_branch_samples(img, locs, size), oracle_samples(img, locs, size))


TIE_DIMS = (64, 16, 16)


def tie_case(n=N_MANY):
    """An inexact sum inside the image that float32 sees.  One bead at x = 7.75 - 2^-50
    (y, z integers): for k >= 1, k + c rounds to k + 7.75, so nlinear's weight is 0.75
    where the bead's own is 0.75 - 2^-50.  The data around it are float32 values in
    [1, 4/3) with odd mantissas: v * 0.75 lies exactly between two floats, v * (0.75 -
    2^-50) just below, and round-to-even takes half of the ties up.  The other beads sit
    at dyadic positions in a region of zeros (exact sums, samples 0), so nothing is added
    to the one bead's samples that could round the difference away."""
    sx, sy, sz = TIE_DIMS
    rng = np.random.default_rng(17)
    img = np.zeros((sz, sy, sx), np.float32)
    m = rng.integers(0, 2 ** 21, (sz, sy, 14)) * 2 + 1                       # odd mantissas, v < 1.25
    img[:, :, 1:15] = (1.0 + m * 2.0 ** -23).astype(np.float32)
    locs = np.stack([rng.integers(30 * 16, 50 * 16, n) / 16.0, rng.integers(5 * 16, 10 * 16, n) / 16.0,
                     rng.integers(6 * 16, 9 * 16, n) / 16.0], axis=1)
    locs[n // 2] = (7.75 - 2.0 ** -50, 8.0, 8.0)
    return img, locs


# ------------------------------------------------------------------ C. chunk loop
C1_SIZE, C1_COUNTS = (3, 3, 3), (65536, 65535 + 32)   # second chunk of 1 bead / of 32 (no remainder)
SMALL_COUNTS = (65, 95, 96, 97)                        # remainders 1, 31, 0, 1 of the 32-wide unroll


@functools.lru_cache(maxsize=None)
def uniform_beads(n, seed=3):
    return image(), np.random.default_rng(seed + n).uniform(-30.0, 40.0, (n, 3))


C2_SIZE, C2_BEADS, C2_IMG = (101, 101, 103), 65, (4, 4, 4)   # 2^26 / 1050703 = 63 beads per chunk


def c2_case():
    """(4 x 4 x 4 image, 65 beads at multiples of 1/8 in [-9, 9)): every k + c is exact, so
    the un-normalised PSF has period 4 per axis around the centre."""
    rng = np.random.default_rng(7)
    return image(C2_IMG, 5), rng.integers(-72, 72, (C2_BEADS, 3)) / 8.0


def c2_expected(size):
    """The oracle's PSF of one centred period (4 x 4 x 4, offsets -2 .. 1), tiled to ``size``
    and then normalised."""
    img, locs = c2_case()
    period = pr.extract_psf_local_batched(img, locs, (4, 4, 4))
    ix = [(np.arange(n) - n // 2 + 2) % 4 for n in size]
    return pr.normalize(period[np.ix_(ix[2], ix[1], ix[0])])


# ------------------------------------------------------------------ D. min / max / normalise
def crop_case(size, values):
    """One bead at integer coordinates in an image that holds its footprint: all weights
    are 1 or 0, so the un-normalised PSF is ``values`` (flat, x fastest) exactly."""
    sx, sy, sz = size
    rng = np.random.default_rng(11)
    img = rng.normal(0, 1, (sz + 3, sy + 3, sx + 3)).astype(np.float32)
    img[1:1 + sz, 1:1 + sy, 1:1 + sx] = np.asarray(values, np.float32).reshape(sz, sy, sx)
    return img, np.array([[1.0 + sx // 2, 1.0 + sy // 2, 1.0 + sz // 2]])


def extremes_case(size, imin, imax):
    """values in (-1, 1) with the only minimum -3 at flat index imin and the only maximum
    5 at imax"""
    n = int(np.prod(size))
    v = np.random.default_rng(12).uniform(-1, 1, n).astype(np.float32)
    v[imin % n], v[imax % n] = -3.0, 5.0
    return crop_case(size, v)


# (size, flat index of the minimum, of the maximum); -1: the last voxel
EXTREMES = [((5, 3, 17), 0, -1), ((5, 3, 17), -1, 0), ((5, 10, 41), 1023, 1024), ((5, 10, 41), 1024, 1023),
            ((5, 10, 41), 2049, 1025), ((3, 3, 3), 13, 26), ((3, 3, 3), 26, 0), ((1, 1, 2), 0, 1)]


def special_image(kind):
    """the small image with NaN / inf voxels, or constant"""
    img = image(seed=9)
    if kind == "nan":
        img[3, 4, 5] = np.nan
    elif kind == "posinf":
        img[3, 4, 5] = np.inf
    elif kind == "neginf":
        img[2, 7, 1] = -np.inf
    elif kind == "bothinf":
        img[3, 4, 5], img[6, 1, 10] = np.inf, -np.inf
    elif kind == "nan_and_inf":
        img[3, 4, 5], img[6, 1, 10] = np.nan, np.inf
    elif kind == "constant":
        img[:] = np.float32(3.25)
    return img


SPECIALS = ["nan", "posinf", "neginf", "bothinf", "nan_and_inf", "constant"]


# ------------------------------------------------------------------ E. transform
def signed_permutation(perm, signs, t=(0, 0, 0)):
    """model with world axis r = signs[r] * source axis perm[r] (+ t[r])"""
    m = np.zeros((3, 4))
    for r in range(3):
        m[r, perm[r]] = signs[r]
        m[r, 3] = t[r]
    return m


def permuted(p, perm, signs):
    """np.transpose / np.flip of [z, y, x] p under signed_permutation (odd sizes: the
    flipped centre stays the centre)"""
    out = np.transpose(p, [2 - perm[2 - a] for a in range(3)])
    for r in range(3):
        if signs[r] < 0:
            out = np.flip(out, axis=2 - r)
    return np.ascontiguousarray(out)


PERMUTATIONS = [((0, 1, 2), (1, 1, 1)), ((1, 0, 2), (1, 1, 1)), ((1, 0, 2), (-1, 1, 1)), ((2, 0, 1), (1, -1, -1)),
                ((0, 1, 2), (-1, -1, -1)), ((2, 1, 0), (1, 1, -1)), ((0, 2, 1), (-1, 1, -1))]


def scale2_expected(p, axis):
    """diag model with 2 on ``axis`` (x = 0): size and offset by the reference's integer
    rule written out, samples at even offsets, float halves at odd ones, 0 past the ends."""
    na = 2 - axis
    n = p.shape[na]
    new = int(2.0 * (n - 1)) + 1
    new += 1 if new % 2 == 0 else 0
    off = 2 * (n // 2) - new // 2
    pm = np.moveaxis(p, na, 0)
    out = np.zeros((new,) + pm.shape[1:], np.float32)
    zero = np.zeros(pm.shape[1:], np.float32)
    at = lambda i: pm[i] if 0 <= i < n else zero   # noqa: E731
    for o in range(new):
        s = o + off
        if s % 2 == 0:
            out[o] = at(s // 2)
        else:
            a, b = at((s - 1) // 2), at((s + 1) // 2)
            out[o] = (a.astype(np.float64) * 0.5).astype(np.float32) + (b.astype(np.float64) * 0.5).astype(np.float32)
    other = [p.shape[2 - d] for d in range(3) if d != axis]
    assert all(m % 2 == 1 for m in other), "odd sizes on the unscaled axes keep them unchanged"
    return np.ascontiguousarray(np.moveaxis(out, 0, na))


# (scaled axis (x = 0), PSF shape [z, y, x]): odd and even sizes on the scaled axis
SCALE2_CASES = [(0, (5, 7, 9)), (0, (5, 7, 8)), (1, (5, 8, 9)), (1, (3, 7, 5)), (2, (8, 5, 7)), (2, (9, 3, 5)),
                (0, (1, 1, 2))]


def scale2_model(axis):
    return np.hstack([np.diag([2.0 if d == axis else 1.0 for d in range(3)]), np.zeros((3, 1))])


def delta_models():
    """six invertible models: rotations with shear and anisotropic scale, one with a
    fractional translation, one shrinking below 1 voxel per axis, one with det < 0"""
    rng = np.random.default_rng(21)
    out = []
    for i in range(6):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a = q @ np.diag(rng.uniform(0.8, 3.0, 3)) @ (np.eye(3) + np.triu(rng.normal(0, 0.2, (3, 3)), 1))
        t = rng.integers(-50, 50, 3).astype(float)
        if i == 1:
            t = t + rng.uniform(0, 1, 3)
        if i == 2:
            a = q @ np.diag([0.4, 0.3, 0.45])
        if i == 3 and np.linalg.det(a) > 0 or i != 3 and np.linalg.det(a) < 0:
            a[:, 0] = -a[:, 0]
        m = np.zeros((3, 4))
        m[:, :3], m[:, 3] = a, t
        out.append(m)
    return out


def delta(size):
    p = np.zeros((size[2], size[1], size[0]), np.float32)
    p[size[2] // 2, size[1] // 2, size[0] // 2] = 1.0
    return p


# size rule: diagonal models on size (11, 11, 11), extent = scale * 10 per axis;
# (scales, expected new size): int(extent) + 1, made odd
SIZE_RULE = [((1.0, 1.5, 0.5), (11, 17, 7)),                                    # integer extents 10; 15 -> 16 -> 17; 5 -> 6 -> 7
             ((1.06, 1.16, 0.96), (11, 13, 11)),                                # 10.6 -> 11; 11.6 -> 12 -> 13; 9.6 -> 10 -> 11
             ((1.1 - 1e-9, 1.2 - 1e-9, 1.0 - 1e-9), (11, 13, 11)),              # just below 11, 12, 10: 10 -> 11, 11 -> 12 -> 13, 9 -> 10 -> 11
             ((0.05, 0.1, 0.15), (1, 3, 3))]                                    # 0.5 -> 1; 1.0 -> 2 -> 3; 1.5 -> 2 -> 3

SHEAR = np.array([[0.8, -0.5, 0.3, 12.5], [0.45, 0.9, -0.2, -7.25], [0.1, 0.35, 3.2, 3.0]])
SHRINK = np.array([[0.35, -0.2, 0.05, 1.0], [0.2, 0.33, 0.1, 2.0], [-0.04, 0.1, 0.4, -3.5]])
ORACLE_MODELS = {"rot": ROT, "shear3.2": SHEAR, "shrink0.4": SHRINK}
ORACLE_SIZES = [(21, 17, 15), (8, 10, 12), (1, 1, 9)]   # PSF array shapes [z, y, x]

SINGULAR = np.array([[1.0, 2.0, 3.0, 0.0], [2.0, 4.0, 6.0, 1.0], [0.0, 1.0, 1.0, 2.0]])
NONFINITE = [np.array([[1.0, 0, 0, 0], [0, np.inf, 0, 0], [0, 0, 1.0, 0]]),
             np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, np.nan, 0]])]


# ------------------------------------------------------------------ F. batches
BATCH_DIMS = [(12, 10, 8), (2, 2, 2), (17, 5, 9), (64, 56, 40), (7, 33, 4)]
BATCH_BEADS = [0, 1, 64, 65, 300]


def batch_case():
    """five views of five different dims (x, y, z) with 0, 1, 64, 65 and 300 beads, models
    alternating ROT / identity"""
    rng = np.random.default_rng(31)
    imgs = [image(d, 40 + v) for v, d in enumerate(BATCH_DIMS)]
    locs = [rng.uniform(-5.0, np.array(d, float) + 5.0, (n, 3)) for d, n in zip(BATCH_DIMS, BATCH_BEADS)]
    models = [ROT if v % 2 == 0 else IDENT for v in range(5)]
    return imgs, locs, models


# ------------------------------------------------------------------ G. projection
def java_max_projection(img, min_dim=-1):
    """computeMaxProjection written as the loop it is (:141-165): running `>` from
    -Double.MAX_VALUE in double, cast to float; independent of oracle.max_projection."""
    dims = [img.shape[2], img.shape[1], img.shape[0]]
    if min_dim < 0:
        min_dim = 0
        for d in range(3):
            if dims[d] < dims[min_dim]:
                min_dim = d
    lines = np.moveaxis(np.asarray(img, np.float32), 2 - min_dim, -1)
    out = np.empty(lines.shape[:2], np.float32)
    for i in range(lines.shape[0]):
        for j in range(lines.shape[1]):
            mx = -np.finfo(np.float64).max
            for v in lines[i, j]:
                if float(v) > mx:
                    mx = float(v)
            with np.errstate(over="ignore"):
                out[i, j] = np.float32(mx)
    return out, min_dim


def projection_volume(shape, seed=51):
    """NaN inside lines, all-NaN lines along every axis, +-inf and ties"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, shape).astype(np.float32)
    v[rng.random(shape) < 0.15] = np.nan
    v[0, :, 0] = np.nan
    v[:, 0, -1] = np.nan
    v[-1, -1, :] = np.nan
    v[shape[0] // 2, shape[1] // 2, shape[2] // 2] = np.inf
    v[0, shape[1] // 2, shape[2] // 2] = -np.inf
    return v


PROJECTION_SHAPES = [(6, 7, 9), (5, 5, 5), (7, 5, 1), (2, 3, 300), (4, 4, 6)]   # [z, y, x]
