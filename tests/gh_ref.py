"""Test helper: restatement of the reference's "fast 3d geometric hashing (rotation invariant)"
candidate stage in NumPy float64 / float32 scalars, operation by operation in the reference's
source order (TEST INFRASTRUCTURE ONLY, like ``oracle/`` and ``tests/rgldm_ref.py``).

    spim/process/interestpointregistration/geometrichashing/GeometricHashingPairwise.java:58-65   fewer than 4
    .../geometrichashing/GeometricHasher.java:54-85        2 nearest B descriptors, the two tests
    .../geometrichashing/GeometricHasher.java:87-116       3 nearest neighbours, normalize = false
    mpicbg/pointdescriptor/AbstractPointDescriptor.java:54-76                 neighbour - basis in double
    mpicbg/pointdescriptor/LocalCoordinateSystemPointDescriptor.java:59-162   buildLocalCoordinateSystem
    .../LocalCoordinateSystemPointDescriptor.java:37-51, :172-175             descriptorDistance, distanceTo
    spim/vecmath/Vector3d.java:127 cross, :157 normalize, :175 dot, :195 length
    spim/vecmath/Matrix3d.java:1212-1263 invertGeneral, :1284-1431 luDecomposition,
                               :1451-1509 luBacksubstitution, :2321-2328 transform(Tuple3d)

Java evaluates ``a * b - c * d`` as two rounded products and one rounded difference; NumPy
scalars do the same, and unlike Python floats they divide by zero into inf / NaN as Java does.

The neighbour search is ``rgldm_ref.descriptors`` (Detection.distanceTo, lower index first on
equal floats).  Unpinned, as fiji.util.KDTree is not in the reference's tree: the B descriptors
are ranked by ``(float) Math.sqrt(descriptorDistance)`` ascending, equal floats by lower B
index, a NaN distance not ranked; with fewer than two ranked the result is Double.MAX_VALUE /
Double.MAX_VALUE / -1 and no candidate.
"""
from __future__ import annotations

import numpy as np

import rgldm_ref as rr

DOUBLE_MAX = rr.DOUBLE_MAX
F64 = np.float64
ZERO, ONE = F64(0.0), F64(1.0)


class SingularMatrixException(Exception):
    pass


# ---------------------------------------------------------------- spim/vecmath/Vector3d
def cross(v1, v2):
    """Vector3d.cross (:127-136)"""
    x = v1[1] * v2[2] - v1[2] * v2[1]
    y = v2[0] * v1[2] - v2[2] * v1[0]
    z = v1[0] * v2[1] - v1[1] * v2[0]
    return [x, y, z]


def normalize(v):
    """Vector3d.normalize() (:157-166)"""
    norm = ONE / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return [v[0] * norm, v[1] * norm, v[2] * norm]


def dot(a, b):
    """Vector3d.dot (:175-178)"""
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def length(v):
    """Vector3d.length (:195-198)"""
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


# ---------------------------------------------------------------- spim/vecmath/Matrix3d
def lu_decomposition(matrix0, row_perm) -> bool:
    """Matrix3d.luDecomposition (:1284-1431) on a list of 9 doubles, in place; False = singular;
    RuntimeError where the reference throws RuntimeException (no pivot found)."""
    row_scale = [ZERO] * 3
    ptr = rs = 0
    for _ in range(3):                       # i = 3; while (i-- != 0)
        big = ZERO
        for _ in range(3):                   # j = 3; while (j-- != 0)
            temp = matrix0[ptr]
            ptr += 1
            temp = abs(temp)
            if temp > big:
                big = temp
        if big == 0.0:
            return False
        row_scale[rs] = ONE / big
        rs += 1
    mtx = 0
    for j in range(3):
        for i in range(j):                   # elements of the upper diagonal matrix U
            target = mtx + 3 * i + j
            s = matrix0[target]
            k = i
            p1 = mtx + 3 * i
            p2 = mtx + j
            while k != 0:
                k -= 1
                s = s - matrix0[p1] * matrix0[p2]
                p1 += 1
                p2 += 3
            matrix0[target] = s
        big = ZERO
        imax = -1
        for i in range(j, 3):                # the largest pivot, elements of L
            target = mtx + 3 * i + j
            s = matrix0[target]
            k = j
            p1 = mtx + 3 * i
            p2 = mtx + j
            while k != 0:
                k -= 1
                s = s - matrix0[p1] * matrix0[p2]
                p1 += 1
                p2 += 3
            matrix0[target] = s
            temp = row_scale[i] * abs(s)
            if temp >= big:
                big = temp
                imax = i
        if imax < 0:
            raise RuntimeError("Matrix3d13")
        if j != imax:                        # exchange rows
            k = 3
            p1 = mtx + 3 * imax
            p2 = mtx + 3 * j
            while k != 0:
                k -= 1
                temp = matrix0[p1]
                matrix0[p1] = matrix0[p2]
                p1 += 1
                matrix0[p2] = temp
                p2 += 1
            row_scale[imax] = row_scale[j]
        row_perm[j] = imax
        if matrix0[mtx + 3 * j + j] == 0.0:
            return False
        if j != 3 - 1:                       # divide elements of L by the pivot
            temp = ONE / matrix0[mtx + 3 * j + j]
            target = mtx + 3 * (j + 1) + j
            i = 2 - j
            while i != 0:
                i -= 1
                matrix0[target] = matrix0[target] * temp
                target += 3
    return True


def lu_backsubstitution(matrix1, row_perm, matrix2):
    """Matrix3d.luBacksubstitution (:1451-1509), matrix2 in place."""
    rp = 0
    for k in range(3):
        cv = k
        ii = -1
        for i in range(3):                   # forward substitution
            ip = row_perm[rp + i]
            s = matrix2[cv + 3 * ip]
            matrix2[cv + 3 * ip] = matrix2[cv + 3 * i]
            if ii >= 0:
                rv = i * 3
                for j in range(ii, i):
                    s = s - matrix1[rv + j] * matrix2[cv + 3 * j]
            elif s != 0.0:
                ii = i
            matrix2[cv + 3 * i] = s
        rv = 2 * 3                           # backsubstitution
        matrix2[cv + 3 * 2] = matrix2[cv + 3 * 2] / matrix1[rv + 2]
        rv -= 3
        matrix2[cv + 3 * 1] = (matrix2[cv + 3 * 1] - matrix1[rv + 2] * matrix2[cv + 3 * 2]) / matrix1[rv + 1]
        rv -= 3
        matrix2[cv + 4 * 0] = (matrix2[cv + 3 * 0] - matrix1[rv + 1] * matrix2[cv + 3 * 1]
                               - matrix1[rv + 2] * matrix2[cv + 3 * 2]) / matrix1[rv + 0]


def invert_general(m):
    """Matrix3d.invertGeneral (:1212-1263): the inverse of the row-major 9 doubles as a new
    list; SingularMatrixException / RuntimeError as the reference."""
    with np.errstate(all="ignore"):
        tmp = [F64(v) for v in m]
        row_perm = [0, 0, 0]
        if not lu_decomposition(tmp, row_perm):
            raise SingularMatrixException("Matrix3d12")
        result = [ZERO] * 9
        result[0] = result[4] = result[8] = ONE
        lu_backsubstitution(tmp, row_perm, result)
        return result


def transform(m, t):
    """Matrix3d.transform(Tuple3d) (:2321-2328)"""
    x = m[0] * t[0] + m[1] * t[1] + m[2] * t[2]
    y = m[3] * t[0] + m[4] * t[1] + m[5] * t[2]
    z = m[6] * t[0] + m[7] * t[1] + m[8] * t[2]
    return [x, y, z]


# ---------------------------------------------------------------- LocalCoordinateSystemPointDescriptor
def build_local_coordinate_system(rel):
    """buildLocalCoordinateSystem (:59-162) with normalize = false over the three relative
    vectors of a point, nearest first: (ax, bx, by, cx, cy, cz) as float32."""
    with np.errstate(all="ignore"):
        b = [F64(v) for v in rel[0]]
        c = [F64(v) for v in rel[1]]
        d = [F64(v) for v in rel[2]]
        x = normalize(d)
        ax = np.float32(length(d))
        n = normalize(cross(b, x))
        if dot(n, c) < 0:
            n = [-n[0], -n[1], -n[2]]
        y = normalize(cross(n, x))
        m = [x[0], y[0], n[0],
             x[1], y[1], n[1],
             x[2], y[2], n[2]]
        zero = np.float32(0.0)
        try:
            m = invert_general(m)
        except (SingularMatrixException, RuntimeError):   # catch ( Exception e )
            return np.array([ax, zero, zero, zero, zero, zero], np.float32)
        bl = transform(m, b)
        cl = transform(m, c)
        return np.array([ax, np.float32(bl[0]), np.float32(bl[1]), np.float32(cl[0]), np.float32(cl[1]),
                         np.float32(cl[2])], np.float32)


def descriptors(points):
    """createLocalCoordinateSystemPointDescriptors (GeometricHasher.java:87-116): (neighbors
    (n, 3) int32, desc (n, 6) float32) of n >= 4 points."""
    nbr, rel = rr.descriptors(points, 3)
    desc = np.empty((len(rel), 6), np.float32)
    for i, r in enumerate(rel):
        desc[i] = build_local_coordinate_system(r)
    return nbr, desc


def descriptor_distance(p, q) -> np.float64:
    """descriptorDistance (:37-51) of two descriptors, literally: float differences, float
    products, each widened and added to a double."""
    with np.errstate(all="ignore"):
        difference = ZERO
        for k in range(6):
            difference = difference + F64((p[k] - q[k]) * (p[k] - q[k]))
        return difference


def descriptor_distances(desc_a, desc_b) -> np.ndarray:
    """descriptor_distance of every A with every B descriptor, vectorised: (na, nb) float64."""
    da, db = np.asarray(desc_a, np.float32), np.asarray(desc_b, np.float32)
    with np.errstate(all="ignore"):
        diff = da[:, None, :] - db[None, :, :]          # float32
        prod = diff * diff                              # float32
        out = np.zeros(prod.shape[:2], np.float64)
        for k in range(6):
            out = out + prod[:, :, k].astype(np.float64)
    return out


def rank_two(row):
    """The ranking rule for one A descriptor over its distances to every B descriptor: B by
    (float) Math.sqrt(distance) ascending, equal floats by lower index, NaN not ranked.
    (best, best index, second), the fill values with fewer than two ranked."""
    with np.errstate(all="ignore"):
        key = np.sqrt(row).astype(np.float32)           # distanceTo (:172-175)
    ranked = np.nonzero(~np.isnan(row))[0]
    if len(ranked) < 2:
        return DOUBLE_MAX, -1, DOUBLE_MAX
    order = ranked[np.argsort(key[ranked], kind="stable")]
    return row[order[0]], int(order[0]), row[order[1]]


def geometric_hashing(pa, pb, ratio_of_distance=10.0, difference_threshold=50.0):
    """GeometricHashingPairwise.call's candidate stage: a dict with neighbors_a / desc_a /
    neighbors_b / desc_b, best_idx / best / second over every A point, and the ordered
    candidates ia, ib."""
    pa = np.asarray(pa, np.float64).reshape(-1, 3)
    pb = np.asarray(pb, np.float64).reshape(-1, 3)
    na = len(pa)
    if na < 4 or len(pb) < 4:                           # "Not enough detections to match"
        return dict(best=np.full(na, DOUBLE_MAX), second=np.full(na, DOUBLE_MAX),
                    best_idx=np.full(na, -1, np.int32), ia=np.zeros(0, np.int32), ib=np.zeros(0, np.int32))
    nbr_a, desc_a = descriptors(pa)
    nbr_b, desc_b = descriptors(pb)
    dist = descriptor_distances(desc_a, desc_b)
    best, second, idx = np.empty(na), np.empty(na), np.empty(na, np.int32)
    for i in range(na):
        best[i], idx[i], second[i] = rank_two(dist[i])
    with np.errstate(all="ignore"):
        keep = (idx >= 0) & (best < F64(difference_threshold)) & (best * F64(ratio_of_distance) <= second)
    ia = np.nonzero(keep)[0].astype(np.int32)
    return dict(neighbors_a=nbr_a, desc_a=desc_a, neighbors_b=nbr_b, desc_b=desc_b, best=best, second=second,
                best_idx=idx, ia=ia, ib=idx[ia])


def candidates(pa, pb, **kw):
    """(ia, ib) of ``geometric_hashing``: the form
    ``registration.pairwise_geometric_hashing(candidates=...)`` takes."""
    r = geometric_hashing(pa, pb, **kw)
    return r["ia"], r["ib"]


# ---------------------------------------------------------------- inputs
def rot_y(deg: float) -> np.ndarray:
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def make_pair(seed: int, na: int, nb: int, box: float = 300.0, noise: float = 0.02, angle: float = 45.0):
    """(A, B): A random in the box; three quarters of B (as far as A reaches) are points of A
    rotated by ``angle`` degrees about y and shifted, plus ``noise`` per coordinate, the rest
    unrelated; B shuffled.  Read-only, so tests can share them."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, box, (na, 3))
    k = min(na, (3 * nb) // 4)
    twin = a[rng.permutation(na)[:k]] @ rot_y(angle).T + np.array([13.0, -21.0, 8.0]) + rng.uniform(-noise, noise,
                                                                                                      (k, 3))
    b = np.concatenate([twin, rng.uniform(0.0, box, (nb - k, 3))])[rng.permutation(nb)]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


A_TILE, B_TILE = 256, 256
# (seed, na, nb) of the pairs the GPU tests run: one below / at / above the A tile and the B
# tile independently, the minimum, one A tile against several B tiles, 257 x 130, a size at
# which the automatic split takes more than one partition, lists below 4; their freedom from
# kNN ties is checked on the CPU (tests/test_gh_cpu.py)
PAIR_CASES = ([(500 + 10 * i + j, na, nb) for i, na in enumerate((A_TILE - 1, A_TILE, A_TILE + 1))
               for j, nb in enumerate((B_TILE - 1, B_TILE, B_TILE + 1))]
              + [(601, 4, 4), (602, 200, 3 * B_TILE + 40), (603, 257, 130), (604, 300, 333), (605, 520, 1100),
                 (606, 3, 5), (607, 5, 3), (608, 2, 2)])
SPLIT_CASE = (604, 300, 333)


def jittered_twins(seed: int, n: int, jitter: float = 4.0):
    """(A, B): A on a 1/64 grid; B = A' + t followed by A' + t + t2 with A' = A moved per
    coordinate by up to ``jitter`` / 64 in 1/64 steps and integer t, t2 (every difference
    exact): each A descriptor meets two bitwise identical B descriptors, n apart, at a
    distance that is not zero."""
    rng = np.random.default_rng(seed)
    a = np.round(rng.uniform(0.0, 300.0, (n, 3)) * 64) / 64
    a2 = a + rng.integers(-int(jitter), int(jitter) + 1, (n, 3)) / 64.0
    b = np.concatenate([a2 + [5.0, 7.0, -3.0], a2 + [1005.0, 7.0, -3.0]])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


TWIN_CASE = (620, 90)


def near_twins(seed: int = 1, n: int = 80, eps: float = 2.0 ** -22):
    """(A, B) as ``jittered_twins`` in a box of 120, but the second copy in B is off by up to
    ``eps`` per coordinate: a few descriptor floats differ in their last bits, so for some A
    points the two copies lie at different double distances whose float roots are equal --
    the case in which the ranking rule (lower index first), not the distance, decides."""
    rng = np.random.default_rng(seed)
    a = np.round(rng.uniform(0.0, 120.0, (n, 3)) * 64) / 64
    a2 = a + rng.integers(-4, 5, (n, 3)) / 64.0
    a3 = a2 + rng.integers(-1, 2, (n, 3)) * eps
    b = np.concatenate([a2 + [5.0, 7.0, -3.0], a3 + [1005.0, 7.0, -3.0]])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def registration_scene(seed: int = 700, views: int = 4, common: int = 300, own: int = 30,
                       angles=(0.0, 45.0, 90.0, 135.0)):
    """``views`` point sets for ``registration.register(matching="geometric_hashing")``: each
    sees a random 85 % of ``common`` world points and ``own`` unrelated ones, in its own frame
    under a known rigid view -> world model (rotation about y by ``angles``, a shift; view 0
    the identity).  Returns (points per view, true models, given models): the given models
    are all the identity, so nothing about the rotations is known."""
    rng = np.random.default_rng(seed)
    world = rng.uniform(0.0, 300.0, (common, 3))
    pts, true, given = [], [], []
    for v in range(views):
        m = np.hstack([np.eye(3), np.zeros((3, 1))])
        if v:
            m[:, :3] = rot_y(angles[v])
            m[:, 3] = rng.uniform(-40, 40, 3)
        seen = world[rng.permutation(common)[:(common * 85) // 100]]
        w = np.concatenate([seen, rng.uniform(0.0, 300.0, (own, 3))])[rng.permutation(len(seen) + own)]
        pts.append((w - m[:, 3]) @ np.linalg.inv(m[:, :3]).T)     # view frame: model(p) = w
        true.append(m)
        given.append(np.hstack([np.eye(3), np.zeros((3, 1))]))
    return pts, true, given
