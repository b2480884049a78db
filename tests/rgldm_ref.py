"""Test helper: NumPy float64 restatement of the reference's "redundant geometric local
descriptor matching" candidate stage, in its operation order (TEST INFRASTRUCTURE ONLY, like
``oracle/`` and ``tests/dom_ref.py``).

    spim/process/interestpointregistration/geometricdescriptor/RGLDMMatcher.java:44-95    best / second, ratio test
    .../geometricdescriptor/RGLDMMatcher.java:97-123                                     nn + re nearest neighbours
    .../geometricdescriptor/RGLDMPairwise.java:46-54                                     "Not enough detections"
    spim/process/interestpointregistration/Detection.java:96-117                         the float kNN metric
    mpicbg/pointdescriptor/AbstractPointDescriptor.java:63-76, :84-112                   neighbour - basis; min over pairings
    mpicbg/pointdescriptor/matcher/SubsetMatcher.java:46-66, :79-107                     a-major pairings, computePD
    mpicbg/pointdescriptor/similarity/SquareDistance.java:11-21                          sum of squareDistance / 3.0

The neighbour search of the reference is a kd-tree whose source is not in its tree: the order
of two neighbours at the same float distance is unpinned (here: lower index first, as the
library).  ``assert_no_knn_ties`` keeps test inputs away from that case.
"""
from __future__ import annotations

import numpy as np

DOUBLE_MAX = np.finfo(np.float64).max   # Double.MAX_VALUE


def compute_pd(n: int, k: int, offset: int = 0):
    """SubsetMatcher.computePD(n, k, offset) (:79-107): the k-subsets of offset .. offset+n-1,
    each ascending, in lexicographic order."""
    cur = [i + offset for i in range(k)]
    out = [list(cur)]
    last = n - k + offset
    while True:
        i = k - 1
        while i >= 0 and cur[i] == last + i:
            i -= 1
        if i < 0:
            return out
        cur[i] += 1
        for j in range(i + 1, k):
            cur[j] = cur[j - 1] + 1
        out.append(list(cur))


def knn_distances(points) -> np.ndarray:
    """Detection.distanceTo for every pair (:96-117): coordinates rounded to float32, the
    per-axis difference in float32 arithmetic, x*x + y*y + z*z and the root in double, the
    result cast to float32.  (n, n) float32."""
    f = np.asarray(points, np.float64).reshape(-1, 3).astype(np.float32)
    d = (f[None, :, :] - f[:, None, :]).astype(np.float64)   # float32 subtraction, then widened
    s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    return np.sqrt(s).astype(np.float32)


def assert_no_knn_ties(points, m: int):
    """No two of a point's m + 1 nearest others (the kept m and the first one left out) lie
    at the same float distance: the unpinned tie order cannot decide anything."""
    d = knn_distances(points)
    np.fill_diagonal(d, np.inf)
    s = np.sort(d, axis=1)[:, :min(m + 1, d.shape[1] - 1)]
    assert np.all(np.diff(s, axis=1) > 0), "input has a float-distance tie among the nearest neighbours"


def descriptors(points, m: int):
    """createSimplePointDescriptors (:97-123): per point the m nearest others in ascending
    float distance (equal distances: lower index first), and neighbour minus basis in double
    (AbstractPointDescriptor.java:63-76).  (n, m) int32, (n, m, 3) float64."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    d = knn_distances(p)
    np.fill_diagonal(d, np.inf)                       # the first hit, the point itself, is dropped
    nbr = np.argsort(d, axis=1, kind="stable")[:, :m].astype(np.int32)
    rel = p[nbr] - p[:, None, :]
    return nbr, rel


def descriptor_distances(rel_a, rel_b, nn: int, chunk: int = 128) -> np.ndarray:
    """descriptorDistance of every A with every B descriptor (AbstractPointDescriptor.java:
    84-112): over SubsetMatcher's pairings in a-major order, similarity = (sum over i of
    squareDistance(a[ca[i]], b[cb[i]])) / 3.0 with a normalisation factor of 1, the smallest
    kept from Double.MAX_VALUE down by strict <.  (na, nb) float64."""
    rel_a, rel_b = np.asarray(rel_a, np.float64), np.asarray(rel_b, np.float64)
    m = rel_a.shape[1]
    comb = compute_pd(m, nn)
    out = np.empty((len(rel_a), len(rel_b)))
    for a0 in range(0, len(rel_a), chunk):
        ra = rel_a[a0:a0 + chunk]
        # Point.squareDistance of neighbour p of A and neighbour q of B: dx*dx + dy*dy + dz*dz
        d = ra[:, None, :, None, :] - rel_b[None, :, None, :, :]           # [A, B, p, q, xyz]
        sq = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        best = np.full(sq.shape[:2], DOUBLE_MAX)
        for ca in comb:
            for cb in comb:
                s = np.zeros(sq.shape[:2])
                for i in range(nn):
                    s = s + sq[:, :, ca[i], cb[i]]
                sim = s / 3.0
                best = np.where(sim < best, sim, best)
        out[a0:a0 + chunk] = best
    return out


def best_second_literal(row):
    """findCorrespondingDescriptors' loop over the B descriptors for one A descriptor
    (RGLDMMatcher.java:54-81), literally: (best, best index or -1, second)."""
    best = second = DOUBLE_MAX
    best_i = second_i = -1
    for j, diff in enumerate(row):
        if diff < second:
            second, second_i = diff, j
            if second < best:
                best, second = second, best
                best_i, second_i = second_i, best_i
    return best, best_i, second


def best_second(dist):
    """best_second_literal over every row, vectorised: the smallest value and the lowest
    index attaining it, and the second smallest of the multiset (values not below
    Double.MAX_VALUE never enter)."""
    d = np.where(dist < DOUBLE_MAX, dist, DOUBLE_MAX)
    idx = np.argmin(d, axis=1).astype(np.int32)       # the first occurrence
    best = d[np.arange(len(d)), idx]
    idx = np.where(best < DOUBLE_MAX, idx, -1).astype(np.int32)
    second = np.partition(d, 1, axis=1)[:, 1] if d.shape[1] > 1 else np.full(len(d), DOUBLE_MAX)
    return best, idx, second


def rgldm(pa, pb, num_neighbors=3, redundancy=1, ratio_of_distance=3.0, difference_threshold=50.0):
    """RGLDMPairwise.call's candidate stage: a dict with neighbors_a / rel_a / neighbors_b /
    rel_b, best_idx / best / second over every A point, and the ordered candidates ia, ib.
    The two thresholds are floats in the reference (RGLDMParameters), widened at use."""
    pa = np.asarray(pa, np.float64).reshape(-1, 3)
    pb = np.asarray(pb, np.float64).reshape(-1, 3)
    m = num_neighbors + redundancy
    na = len(pa)
    if na < m + 1 or len(pb) < m + 1:                 # "Not enough detections to match"
        return dict(best=np.full(na, DOUBLE_MAX), second=np.full(na, DOUBLE_MAX),
                    best_idx=np.full(na, -1, np.int32), ia=np.zeros(0, np.int32), ib=np.zeros(0, np.int32))
    nbr_a, rel_a = descriptors(pa, m)
    nbr_b, rel_b = descriptors(pb, m)
    best, idx, second = best_second(descriptor_distances(rel_a, rel_b, num_neighbors))
    thr, ratio = np.float64(np.float32(difference_threshold)), np.float64(np.float32(ratio_of_distance))
    keep = (best < thr) & (best * ratio < second)
    ia = np.nonzero(keep)[0].astype(np.int32)
    return dict(neighbors_a=nbr_a, rel_a=rel_a, neighbors_b=nbr_b, rel_b=rel_b, best=best, second=second,
                best_idx=idx, ia=ia, ib=idx[ia])


def candidates(pa, pb, **kw):
    """(ia, ib) of ``rgldm``: the form ``registration.pairwise_rgldm(candidates=...)`` takes."""
    r = rgldm(pa, pb, **kw)
    return r["ia"], r["ib"]


def random_points(seed: int, n: int, box: float = 300.0) -> np.ndarray:
    """n points with continuous coordinates in a box a few hundred wide."""
    p = np.random.default_rng(seed).uniform(0.0, box, (n, 3))
    p.setflags(write=False)
    return p


def make_pair(seed: int, na: int, nb: int, box: float = 300.0, noise: float = 0.2):
    """(A, B): A random in the box; three quarters of B (as far as A reaches) are points of A
    moved by one translation plus ``noise`` per coordinate, the rest unrelated; B shuffled.
    Read-only, so tests can share them."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, box, (na, 3))
    k = min(na, (3 * nb) // 4)
    twin = a[rng.permutation(na)[:k]] + np.array([13.0, -21.0, 8.0]) + rng.uniform(-noise, noise, (k, 3))
    b = np.concatenate([twin, rng.uniform(0.0, box, (nb - k, 3))])[rng.permutation(nb)]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def twin_clusters(seed: int, n: int):
    """(A, B): A on a 1/64 grid, B = A + t followed by A + t + t2 with integer t, t2 (every
    difference exact): each A descriptor has two identical B descriptors, n apart."""
    a = np.round(np.random.default_rng(seed).uniform(0.0, 300.0, (n, 3)) * 64) / 64
    b = np.concatenate([a + [5.0, 7.0, -3.0], a + [1005.0, 7.0, -3.0]])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


# (seed, na, nb) of the pairs the GPU tests run (A tile 128, B tile 64); their freedom from
# kNN ties is checked on the CPU (tests/test_rgldm_cpu.py)
PAIR_CASES = ([(200 + 10 * i + j, na, nb) for i, na in enumerate((127, 128, 129)) for j, nb in enumerate((63, 64, 65))]
              + [(301, 5, 5), (302, 4, 5), (303, 5, 4), (304, 257, 130), (305, 128, 400), (306, 200, 333),
                 (307, 150, 140), (308, 7, 7), (309, 2, 2), (310, 1500, 1900)])
TWIN_CASE = (320, 90)


def _rot(axis, angle):
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def registration_scene(kind: str, noise: float, seed: int = 400, views: int = 4, common: int = 300, own: int = 100):
    """``views`` point sets for ``registration.register``: each sees a random 85 % of
    ``common`` world points (plus ``noise`` per coordinate) and ``own`` unrelated ones, in its
    own frame under a known view -> world model of ``kind`` (view 0: the identity).  Returns
    (points per view, true models, given models): the given models are the true ones off by
    5-30 px per axis (view 0 exact), far outside a 2 px nearest-detection radius."""
    rng = np.random.default_rng(seed)
    world = rng.uniform(0.0, 300.0, (common, 3))
    pts, true, given = [], [], []
    for v in range(views):
        m = np.hstack([np.eye(3), np.zeros((3, 1))])
        if v:
            if kind == "rigid":
                m[:, :3] = _rot(rng.normal(size=3), 0.3 * v)
            elif kind == "affine":
                m[:, :3] = _rot(rng.normal(size=3), 0.3 * v) @ (np.eye(3) + rng.uniform(-0.05, 0.05, (3, 3)))
            m[:, 3] = rng.uniform(-40, 40, 3)
        seen = world[rng.permutation(common)[:(common * 85) // 100]]
        w = np.concatenate([seen + rng.uniform(-noise, noise, seen.shape) if noise else seen,
                            rng.uniform(0.0, 300.0, (own, 3))])[rng.permutation(len(seen) + own)]
        inv = np.linalg.inv(m[:, :3])
        pts.append((w - m[:, 3]) @ inv.T)                     # view frame: model(p) = w
        g = m.copy()
        if v:
            g[:, 3] += rng.uniform(5, 30, 3) * rng.choice([-1, 1], 3)
        true.append(m)
        given.append(g)
    return pts, true, given
