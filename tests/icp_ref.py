"""Test helper: restatement of the reference's "Iterative closest-point (ICP, no invariance)"
matcher in NumPy float64 / float32, operation by operation in the reference's source order
(TEST INFRASTRUCTURE ONLY, like ``oracle/``, ``tests/rgldm_ref.py`` and ``tests/gh_ref.py``).

    spim/process/interestpointregistration/icp/IterativeClosestPointPairwise.java:40-122   the loop
    .../icp/IterativeClosestPointParameters.java            max distance 5, max iterations 100
    mpicbg/icp/ICP.java:91-115                              runICPIteration
    mpicbg/icp/ICP.java:208-317                             removeAmbigousMatches, getOccurences
    mpicbg/icp/SimplePointMatchIdentification.java:32-48    nearest target per reference point
    spim/process/interestpointregistration/Detection.java:96-115   distanceTo, get

List A is the target (its points are moved by the model), list B the reference.  NumPy's
elementwise ``a * b + c`` is two rounded operations, as Java's.

Unpinned, as fiji.util.KDTree and mpicbg's models are not in the reference's tree: among equal
float distances the lower target index is the nearest; ``fit`` is ``globalopt.fit``.
"""
from __future__ import annotations

import numpy as np

from spim_registration_amd import globalopt

F32, F64 = np.float32, np.float64
FLOAT_MAX = np.finfo(np.float32).max
R_BLOCK, T_TILE = 256, 1024      # csrc/icp.hip: reference points per block, target points per LDS tile


def identity():
    return np.hstack([np.eye(3), np.zeros((3, 1))])


def apply(model, pts) -> np.ndarray:
    """Point.apply(model) for an (n, 3) list: per row ((m0 x + m1 y) + m2 z) + m3, every product
    and sum rounded on its own."""
    m = identity() if model is None else np.asarray(model, F64).reshape(3, 4)
    p = np.asarray(pts, F64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    return out


def distance_to(t, o) -> np.ndarray:
    """Detection.distanceTo (:96-103) of target points ``t`` towards reference points ``o``
    (world coordinates in double, broadcast over the leading axes): get(k) = (float) w[k], the
    differences o.get(k) - get(k) in float, widened; x*x + y*y + z*z and the root in double;
    the cast to float."""
    tf, of = np.asarray(t, F64).astype(F32), np.asarray(o, F64).astype(F32)
    with np.errstate(all="ignore"):
        d = (of - tf).astype(F64)
        x, y, z = d[..., 0], d[..., 1], d[..., 2]
        return np.sqrt(x * x + y * y + z * z).astype(F32)


def distance_sums(t, o) -> np.ndarray:
    """the double under ``distance_to``'s root"""
    tf, of = np.asarray(t, F64).astype(F32), np.asarray(o, F64).astype(F32)
    d = (of - tf).astype(F64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return x * x + y * y + z * z


def distances(target_w, reference) -> np.ndarray:
    """the full (|reference|, |target|) float matrix"""
    return distance_to(np.asarray(target_w, F64)[None, :, :], np.asarray(reference, F64)[:, None, :])


def remove_ambiguous_literal(matches):
    """ICP.removeAmbigousMatches (:208-249) with getOccurences (:259-317) as written, over a list
    of (target index, reference index) -- object identity is index equality.  Returns (the
    matches left, the removed ones in the order the reference collects them)."""
    matches = list(matches)

    def occurences(t, r):
        occ = []
        different = False
        for pt, pr in matches:
            if pr == r and pt != t:
                different = True
                break
            if pt == t and pr != r:
                different = True
                break
        if different:
            for i, (pt, pr) in enumerate(matches):
                if pr == r:
                    occ.append(i)
                if pt == t:
                    occ.append(i)
        else:
            same = False
            for i, (pt, pr) in enumerate(matches):
                if pr == r:
                    if same:
                        occ.append(i)
                    else:
                        same = True
        return occ

    inconsistent = []
    for i in range(len(matches)):
        t, r = matches[i]
        for index in occurences(t, r):
            if index not in inconsistent:
                inconsistent.append(index)
    removed = []
    if inconsistent:
        inconsistent.sort()
        for i in range(len(inconsistent) - 1, -1, -1):
            removed.append(matches[inconsistent[i]])
            del matches[inconsistent[i]]
    return matches, removed


def remove_ambiguous(it, ir):
    """The claim-count form for reference points that occur once each: a match goes when
    another match names its target.  Returns (it, ir, the number removed)."""
    it, ir = np.asarray(it, np.int32), np.asarray(ir, np.int32)
    claims = np.bincount(it, minlength=1)
    keep = claims[it] == 1
    return it[keep], ir[keep], int((~keep).sum())


def assign(target, reference, model=None, max_distance=5.0, device=0, return_all=False, t_split=0):
    """``registration.icp_assign``'s signature and result: apply, SimplePointMatchIdentification
    over the full float matrix (argmin: the first index on ties), the threshold
    (double) dist <= (double)(float) maxDistance, removeAmbigousMatches."""
    target = np.asarray(target, F64).reshape(-1, 3)
    reference = np.asarray(reference, F64).reshape(-1, 3)
    nt, nr = len(target), len(reference)
    if nt == 0:
        nearest, dist = np.full(nr, -1, np.int32), np.full(nr, FLOAT_MAX, F32)
        matched = np.zeros(nr, bool)
    else:
        d = distances(apply(model, target), reference)
        nearest = np.argmin(d, axis=1).astype(np.int32)
        dist = d[np.arange(nr), nearest]
        matched = dist.astype(F64) <= F64(F32(max_distance))
    ir = np.nonzero(matched)[0].astype(np.int32)
    it, ir, ambiguous = remove_ambiguous(nearest[ir], ir)
    return (it, ir, nearest, dist, ambiguous) if return_all else (it, ir)


def icp(pa, pb, model="affine", max_distance=5.0, max_iterations=100):
    """IterativeClosestPointPairwise.call (:40-122) as its do-while: (it, ir, model or None,
    avgError or NaN, i)."""
    pa, pb = np.asarray(pa, F64).reshape(-1, 3), np.asarray(pb, F64).reshape(-1, 3)
    none = np.zeros(0, np.int32)
    least = globalopt.MIN_MATCHES[model]
    if len(pa) < least or len(pb) < least:
        return none, none, None, float("nan"), 0
    m = identity()
    i, last_err, last_n, converged = 0, 0.0, 0, False
    while True:
        it, ir = assign(pa, pb, m, max_distance)
        try:
            m = globalopt.fit(model, pa[it], pb[ir], np.ones(len(it)))
        except (globalopt.NotEnoughDataPoints, globalopt.IllDefinedDataPoints):
            return none, none, None, float("nan"), i
        d = np.linalg.norm(globalopt.apply(m, pa[it]) - pb[ir], axis=1)
        avg, n = float(d.mean()), len(it)
        if last_n == n and last_err == avg:
            converged = True
        last_n, last_err = n, avg
        if converged:
            break
        i += 1
        if not i < max_iterations:
            break
    return it, ir, m, avg, i


# ---------------------------------------------------------------- inputs
def rot_z(deg: float) -> np.ndarray:
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


AFFINE = np.array([[0.98, 0.05, -0.03, 13.0], [-0.04, 1.03, 0.02, -21.0], [0.01, -0.06, 0.97, 8.0]])


def make_case(seed: int, nt: int, nr: int, model=None, box: float = 300.0, noise: float = 0.5):
    """(target, reference): the target random in the box; six tenths of the reference points are
    target points (drawn with replacement, so some targets are taken twice or more: ambiguous
    claims) under ``model`` plus ``noise`` per coordinate, the rest unrelated points of the
    box under ``model`` (mostly farther than 5 from every target).  Read-only."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, box, (nt, 3))
    k = (6 * nr) // 10
    twin = t[rng.integers(0, nt, k)] + rng.uniform(-noise, noise, (k, 3))
    r = np.concatenate([twin, rng.uniform(0.0, box, (nr - k, 3))])[rng.permutation(nr)]
    r = apply(model, r)
    t.setflags(write=False)
    r.setflags(write=False)
    return t, r


# (seed, nt, nr) of the pairs the GPU tests run: the reference list one below / at / above the
# block and the target list one below / at / above the tile independently, 1 x 1, one target,
# one reference point, and two with several target tiles against few reference blocks, where
# the automatic split takes more than one partition
SIZE_CASES = ([(800 + 10 * i + j, nt, nr) for i, nr in enumerate((R_BLOCK - 1, R_BLOCK, R_BLOCK + 1))
               for j, nt in enumerate((T_TILE - 1, T_TILE, T_TILE + 1))]
              + [(901, 1, 1), (902, 1, 300), (903, 300, 1), (904, 3 * T_TILE + 40, 520), (905, 2500, 300)])
SPLIT_CASE = (906, 333, 300)


def lattice_case():
    """(target, reference): a 4 x 4 x 4 integer lattice and the 27 cell centres: each centre has
    its eight corners at exactly the same float distance."""
    g = np.arange(4.0)
    t = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    c = np.arange(3.0) + 0.5
    r = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    return t, r


def equal_float_case(n: int = 12):
    """(target, reference): reference point k at (100 k, 0, 0) with two targets at (3, 4, 2^-10)
    and (3, 4, 0) from it: 25 + 2^-20 and 25 in double, 5.0f both.  For even k the farther
    target has the lower index, for odd k the nearer one."""
    r = np.zeros((n, 3))
    r[:, 0] = 100.0 * np.arange(n)
    far, near = r + [3.0, 4.0, 2.0 ** -10], r + [3.0, 4.0, 0.0]
    t = np.empty((2 * n, 3))
    t[0::2] = np.where((np.arange(n) % 2 == 0)[:, None], far, near)
    t[1::2] = np.where((np.arange(n) % 2 == 0)[:, None], near, far)
    return t, r


def ambiguity_case():
    """(target, reference, the surviving (it, ir), the ambiguous count) at max_distance 5: two
    reference points share target 0, three share target 1 -- all five removed; target 2 is the
    nearest of two more, one of them 7 away: beyond the threshold it claims nothing, the other
    survives; target 3 is matched once."""
    t = np.array([[0.0, 0, 0], [100.0, 0, 0], [200.0, 0, 0], [300.0, 0, 0]])
    r = np.array([[1.0, 0, 0], [100.0, 2, 0], [200.0, 7, 0], [0.0, 1, 0], [101.0, 0, 0], [201.0, 0, 0],
                  [100.0, 0, -3], [300.0, 0, 1]])
    return t, r, (np.array([2, 3], np.int32), np.array([5, 7], np.int32)), 5


def fma_cases():
    """[(model, target, reference)]: one target
    whose x row is m0 x + 1 y with m0 x = 2^20 + ... inexact and y cancelling it down to a
    double exactly between two floats.  Rounded separately the sum is that midpoint (the float
    cast goes to even); fused, the product's lost bits decide the cast the other way.  The
    reference point is the origin and the other rows give 0, so dist is the x float itself."""
    out = []
    for m0, mid in ((1.0 + 2.0 ** -30, 1.0 + 2.0 ** -24), (1.0 - 2.0 ** -30, 1.0 + 3 * 2.0 ** -24)):
        x = 2.0 ** 20 + 2.0 ** -10
        y = mid - float(F64(m0) * F64(x))
        model = np.array([[m0, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, -y], [0.0, 0.0, 1.0, 0.0]])
        out.append((model, np.array([[x, y, 0.0]]), np.zeros((1, 3))))
    return out


RECOVERY_MOTION = np.hstack([rot_z(1.0), np.array([[1.5], [-1.0], [0.5]])])


FAR_MOTION = np.hstack([rot_z(3.0), np.array([[3.0], [-2.0], [1.0]])])   # most points start beyond 5 px


def recovery_case(seed: int = 954, n: int = 300, box: float = 300.0, noise: float = 0.1, outliers: float = 0.3,
                  motion=RECOVERY_MOTION):
    """(A, B): A random in the box; B = A under ``motion`` plus Gaussian noise; then 30 % of
    each list (chosen independently) replaced by unrelated points of the box.  (The seed is one
    at which the identity's assignment holds ambiguous claims: tests/test_icp_cpu.py.)"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, box, (n, 3))
    b = globalopt.apply(motion, a) + rng.normal(0.0, noise, (n, 3))
    k = int(n * outliers)
    a[rng.permutation(n)[:k]] = rng.uniform(0.0, box, (k, 3))
    b[rng.permutation(n)[:k]] = rng.uniform(0.0, box, (k, 3))
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def registration_scene(seed: int = 970, views: int = 4, common: int = 400, own: int = 0, noise: float = 0.01):
    """``views`` point sets for ``registration.register_icp``: each sees a random 85 % of
    ``common`` world points (plus ``noise`` per coordinate) and ``own`` unrelated ones, in its
    own frame under a rigid view -> world model.  (One bead set, no unrelated detections: ICP
    rejects by distance alone, and an unrelated point within 5 px of a bead, 3 px off among 300
    matches, moves a translation by 1e-2.)  Returns (points per view, true models, given
    models): the given models are the true ones followed by a rotation of up to 1 degree about
    the box centre and a shift of up to 2 px (view 0 exact)."""
    rng = np.random.default_rng(seed)
    world = rng.uniform(0.0, 300.0, (common, 3))
    centre = np.full(3, 150.0)
    pts, true, given = [], [], []
    for v in range(views):
        m = identity()
        if v:
            m[:, :3] = rot_z(20.0 * v)
            m[:, 3] = rng.uniform(-40, 40, 3)
        seen = world[rng.permutation(common)[:(common * 85) // 100]]
        w = np.concatenate([seen + rng.uniform(-noise, noise, seen.shape),
                            rng.uniform(0.0, 300.0, (own, 3))])[rng.permutation(len(seen) + own)]
        pts.append((w - m[:, 3]) @ np.linalg.inv(m[:, :3]).T)     # view frame: model(p) = w
        g = m.copy()
        if v:
            rot = rot_z(rng.uniform(0.5, 1.0) * rng.choice([-1, 1]))
            shift = rng.uniform(1.0, 2.0, 3) * rng.choice([-1, 1], 3) / np.sqrt(3.0)
            off = np.hstack([rot, (centre - rot @ centre + shift)[:, None]])
            g = globalopt.concatenate(off, m)
        true.append(m)
        given.append(g)
    return pts, true, given
