"""Restatement of the reference's reorienting bounding box in float64, operation by operation:
spim/process/fusion/boundingbox/AutomaticReorientation.java with the vendored vecmath
(spim/vecmath/Transform3D.java:1397-1450 set(AxisAngle4d), :4755-4765 transform(Point3d),
Vector3d.java:127-166 cross / normalize).  Python floats and NumPy float64 arrays: every product,
sum and difference is rounded on its own (nothing is contracted), in the Java source order.

Not pinned against a JVM: Java's Math.sin / Math.cos / Math.acos may differ from the host libm
(which ``math`` calls) by an ulp, and imglib2's AffineTransform3D.apply -- behind
``world_points`` and the preconcatenation -- is not in the reference tree; its rows are taken
as the left-to-right sums m0 x + m1 y + m2 z + m3.
"""
import math
import sys

import numpy as np

DOUBLE_MAX = sys.float_info.max                     # Double.MAX_VALUE
VECTOR_STEPS = (0.4, 0.2, 0.1, 0.05, 0.025, 0.01, 0.005, 0.001)   # :353
EPSILON_ABSOLUTE = 1.0e-5                           # Transform3D.java:154
X_AXIS = (1.0, 0.0, 0.0)


# ---------------------------------------------------------------- Math.*
def java_min(a, b):
    """Math.min(double, double)"""
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, b) < 0.0:
        return b
    return a if a <= b else b


def java_max(a, b):
    """Math.max(double, double)"""
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, a) < 0.0:
        return b
    return a if a >= b else b


def java_round(x):
    """Math.round(double) as floor(x + 0.5) saturated to a long (NaN: 0)"""
    if x != x:
        return 0
    f = math.floor(x + 0.5) if math.isfinite(x) else (2 ** 63 if x > 0 else -2 ** 63)
    return max(-2 ** 63, min(2 ** 63 - 1, f))


def java_int(v):
    """the (int) cast of a long: the low 32 bits"""
    return ((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31


def _acos(x):
    return math.acos(x) if -1.0 <= x <= 1.0 else math.nan      # Math.acos: NaN outside [-1, 1]


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else math.nan


def _recip(x):
    if x == 0.0:
        return math.copysign(math.inf, x)
    return 1.0 / x


# ---------------------------------------------------------------- :514-573
def world_points(lists, models, corresponding=None, detections=None):
    """getAllDetectionsInGlobalCoordinates: the lists in view order, every row of a model as the
    left-to-right sum m0 x + m1 y + m2 z + m3.  detections="corresponding" (the default when
    ``corresponding`` is given): only the indices corresponding[v] of list v, in that order."""
    if detections is None:
        detections = "all" if corresponding is None else "corresponding"
    out = []
    for v, (pts, m) in enumerate(zip(lists, models)):
        p = np.asarray(pts, np.float64).reshape(-1, 3)
        if detections == "corresponding":
            p = p[np.asarray(corresponding[v], np.int64).reshape(-1)]
        m = np.asarray(m, np.float64).reshape(3, 4)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        out.append(np.stack([m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(3)], axis=1))
    return np.ascontiguousarray(np.concatenate(out)) if out else np.zeros((0, 3))


# ---------------------------------------------------------------- :316-343, :479-486
def square_distance(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return dx * dx + dy * dy + dz * dz


def farthest_pair_literal(points):
    """:316-343 as written, pair by pair (for small lists): (index of p1, index of p2, maxDist)"""
    pts = [tuple(float(c) for c in p) for p in np.asarray(points, np.float64).reshape(-1, 3)]
    p1, p2 = 0, 1
    max_dist = square_distance(pts[0], pts[1])
    for i in range(len(pts) - 1):
        for j in range(i + 1, len(pts)):
            a, b = pts[i], pts[j]
            d = square_distance(a, b)
            if d > max_dist:
                max_dist = d
                if a[0] <= b[0]:
                    p1, p2 = i, j
                else:
                    p1, p2 = j, i
    return p1, p2, max_dist


def farthest_pair(points):
    """:316-343 with the inner loop of a row i taken at once: within a row the strict d > maxDist
    ends at the first j of the row's largest d when that is larger than maxDist, and nowhere
    otherwise -- the same state after every row as ``farthest_pair_literal`` (the tests compare
    the two).  (index of p1, index of p2, maxDist)."""
    pts = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    p1, p2 = 0, 1
    max_dist = square_distance(pts[0], pts[1])
    for i in range(len(pts) - 1):
        dx, dy, dz = pts[i, 0] - pts[i + 1:, 0], pts[i, 1] - pts[i + 1:, 1], pts[i, 2] - pts[i + 1:, 2]
        d = dx * dx + dy * dy + dz * dz
        k = int(np.argmax(d))                 # the first of the row's largest
        if d[k] > max_dist:
            max_dist = d[k]
            j = i + 1 + k
            p1, p2 = (i, j) if pts[i, 0] <= pts[j, 0] else (j, i)
    return p1, p2, float(max_dist)


# ---------------------------------------------------------------- vecmath
def normalize(v):
    """Vector3d.normalize: 1.0 / Math.sqrt(...), then three products"""
    x, y, z = v
    norm = _recip(_sqrt(x * x + y * y + z * z))
    return (x * norm, y * norm, z * norm)


def identity():
    return np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])


def rotation(v0, v1):
    """getRotation :457-477 as the 3x4 head of the Transform3D.  A NaN axis -- parallel, and
    also antiparallel vectors -- gives the identity."""
    ax = (v0[1] * v1[2] - v0[2] * v1[1], v1[0] * v0[2] - v1[2] * v0[0], v0[0] * v1[1] - v0[1] * v1[0])
    ax = normalize(ax)
    if ax[0] != ax[0]:
        return identity()
    angle = _acos(v0[0] * v1[0] + v0[1] * v1[1] + v0[2] * v1[2])
    # Transform3D.set(AxisAngle4d)
    mag = _sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2])
    if mag < EPSILON_ABSOLUTE and mag > -EPSILON_ABSOLUTE:     # almostZero
        return identity()
    mag = _recip(mag)
    x, y, z = ax[0] * mag, ax[1] * mag, ax[2] * mag
    sin_t = math.sin(angle) if angle == angle else math.nan
    cos_t = math.cos(angle) if angle == angle else math.nan
    t = 1.0 - cos_t
    xz, xy, yz = x * z, x * y, y * z
    return np.array([[t * x * x + cos_t, t * xy - sin_t * z, t * xz + sin_t * y, 0.0],
                     [t * xy + sin_t * z, t * y * y + cos_t, t * yz - sin_t * x, 0.0],
                     [t * xz - sin_t * y, t * yz + sin_t * x, t * z * z + cos_t, 0.0]])


def transform_points(mat, points):
    """Transform3D.transform(Point3d) for every point: per row m0 x + m1 y + m2 z + m3"""
    m = np.asarray(mat, np.float64).reshape(3, 4)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(3)], axis=1)


def box_of(coords):
    """the fold of testAxis :421-442: Math.min / Math.max from +-Double.MAX_VALUE, in list
    order; [minX, minY, minZ, maxX, maxY, maxZ]"""
    lo, hi = [DOUBLE_MAX] * 3, [-DOUBLE_MAX] * 3
    for row in np.asarray(coords, np.float64).reshape(-1, 3).tolist():
        for a in range(3):
            lo[a] = java_min(lo[a], row[a])
            hi[a] = java_max(hi[a], row[a])
    return lo + hi


def volume_of(box):
    return (box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2])


def axis_boxes(points, matrices):
    """(m, 6): ``box_of`` under each of the 3x4 ``matrices``"""
    mats = np.asarray(matrices, np.float64).reshape(-1, 3, 4)
    return np.array([box_of(transform_points(m, points)) for m in mats])


def test_axis(v, points):
    """testAxis :413-447: (volume, [minX, minY, minZ, maxX, maxY, maxZ])"""
    box = box_of(transform_points(rotation(v, X_AXIS), points))
    return volume_of(box), box


test_axis.__test__ = False    # (not a pytest case)


# ---------------------------------------------------------------- :306-401
def optimal_bounding_box(points):
    """determineOptimalBoundingBox: a dict with transform (3x4), box (minBoundingBox), far_pair
    (indices of p1, p2), far_d2, start_volume (the volume logged before the search), min_volume
    and axis (the final search vector)."""
    pts = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    i1, i2, max_dist = farthest_pair(pts)
    p1, p2 = pts[i1].tolist(), pts[i2].tolist()
    sv = normalize((p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]))
    start_volume = test_axis(sv, pts)[0]
    min_volume, min_box = DOUBLE_MAX, None
    for step in VECTOR_STEPS:
        best_sv = sv
        for zi in (-1, 0, 1):
            for yi in (-1, 0, 1):
                for xi in (-1, 0, 1):
                    v = normalize((sv[0] + xi * step, sv[1] + yi * step, sv[2] + zi * step))
                    vol, box = test_axis(v, pts)
                    if vol < min_volume:
                        min_volume, min_box, best_sv = vol, box, v
        sv = best_sv
    return {"transform": rotation(sv, X_AXIS), "box": min_box, "far_pair": (i1, i2), "far_d2": max_dist,
            "start_volume": start_volume, "min_volume": min_volume, "axis": sv}


# ---------------------------------------------------------------- :488-512
def size_simple(points):
    """determineSizeSimple: (min, max), from a copy of the first point, Math.min / Math.max"""
    rows = np.asarray(points, np.float64).reshape(-1, 3).tolist()
    lo, hi = list(rows[0]), list(rows[0])
    for row in rows:
        for a in range(3):
            lo[a] = java_min(lo[a], row[a])
            hi[a] = java_max(hi[a], row[a])
    return lo, hi


# ---------------------------------------------------------------- :277-289
def padded_box(min_f, max_f, percent):
    """(min, max) as Java ints: one ``add``, the largest over the axes of (max - min) *
    (percent / 100.0) / 2; (int) Math.round(min - add), (int) Math.round(max + add)"""
    add_x = (max_f[0] - min_f[0]) * (percent / 100.0) / 2
    add_y = (max_f[1] - min_f[1]) * (percent / 100.0) / 2
    add_z = (max_f[2] - min_f[2]) * (percent / 100.0) / 2
    add = java_max(add_x, java_max(add_y, add_z))
    return ([java_int(java_round(min_f[a] - add)) for a in range(3)],
            [java_int(java_round(max_f[a] + add)) for a in range(3)])


def preconcatenate(transform, model):
    """transform o model (ViewRegistration.preconcatenateTransform, :263), element by element as
    the left-to-right sum over the inner index, the translation added last"""
    t = np.asarray(transform, np.float64).reshape(3, 4)
    m = np.asarray(model, np.float64).reshape(3, 4)
    out = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            s = float(t[r, 0]) * float(m[0, c]) + float(t[r, 1]) * float(m[1, c]) + float(t[r, 2]) * float(m[2, c])
            out[r, c] = s + float(t[r, 3]) if c == 3 else s
    return out


def reorient_bounding_box(lists, models, corresponding=None, percent=10.0, reorientate=True):
    """the whole step: a dict with transform, new_models, min_f, max_f, bb_min, bb_max, bb_dims
    and, with ``reorientate``, what ``optimal_bounding_box`` returns"""
    pts = world_points(lists, models, corresponding)
    if reorientate:
        det = optimal_bounding_box(pts)
        transform, min_f, max_f = det["transform"], det["box"][:3], det["box"][3:]
    else:
        det = {}
        transform = identity()
        min_f, max_f = size_simple(pts)
    lo, hi = padded_box(min_f, max_f, percent)
    return {**det, "points": pts, "transform": transform, "min_f": min_f, "max_f": max_f,
            "new_models": [preconcatenate(transform, m) for m in models],
            "bb_min": tuple(lo), "bb_max": tuple(hi), "bb_dims": tuple(h - l + 1 for l, h in zip(lo, hi))}


# ---------------------------------------------------------------- shared cases
def rot_zyx(az, ay, ax_):
    """a plain rotation matrix (test scenes only)"""
    cz, sz, cy, sy, cx, sx = math.cos(az), math.sin(az), math.cos(ay), math.sin(ay), math.cos(ax_), math.sin(ax_)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return rz @ ry @ rx


def axis_rotation(u):
    """the rotation about x cross u that takes the x axis onto the unit vector u (Rodrigues'
    formula in NumPy: independent of ``rotation``): the search only looks for the direction that
    goes onto x, and getRotation fixes the roll about it, so a scene whose box the search can
    find exactly is turned this way"""
    u = np.asarray(u, np.float64) / np.linalg.norm(u)
    k = np.cross([1.0, 0.0, 0.0], u)
    s, c = np.linalg.norm(k), u[0]
    k = k / s
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + s * K + (1.0 - c) * (K @ K)


CUBOID = (200.0, 40.0, 20.0)
CUBOID_AXIS = np.array([0.6, 0.5, -0.62]) / np.linalg.norm([0.6, 0.5, -0.62])
CUBOID_ROT = axis_rotation(CUBOID_AXIS)
CUBOID_SHIFT = np.array([310.0, 120.0, -45.0])


def cuboid_points(n=400, seed=7):
    """n points of a 200 x 40 x 20 cuboid -- its eight corners and n - 8 uniform ones --
    turned by CUBOID_ROT (its long axis onto CUBOID_AXIS) about the origin and shifted: (world points, the cuboid's own volume)"""
    rng = np.random.default_rng(seed)
    corners = np.array([[x, y, z] for x in (0.0, CUBOID[0]) for y in (0.0, CUBOID[1]) for z in (0.0, CUBOID[2])])
    inner = rng.uniform(0.0, 1.0, (n - 8, 3)) * np.array(CUBOID)
    local = np.concatenate([inner[: (n - 8) // 2], corners, inner[(n - 8) // 2:]])
    return np.ascontiguousarray(local @ CUBOID_ROT.T + CUBOID_SHIFT), CUBOID[0] * CUBOID[1] * CUBOID[2]


def cuboid_views():
    """the cuboid's 400 world points split over 3 views with non-trivial models: per view the
    detections in view pixels (world points through the inverse model, so the world points are
    recovered to rounding), the models, and per view the indices of a "corresponding" subset,
    unsorted"""
    world, _ = cuboid_points()
    rng = np.random.default_rng(11)
    cuts = [0, 150, 270, 400]
    lists, models, corr = [], [], []
    for v in range(3):
        a = rot_zyx(0.3 * v, 0.5 - 0.2 * v, -0.1 * v) * (1.0 + 0.05 * v)
        t = np.array([12.5 * v, -7.25, 3.0 + v])
        m = np.concatenate([a, t[:, None]], axis=1)
        w = world[cuts[v]:cuts[v + 1]]
        lists.append(np.ascontiguousarray((w - t) @ np.linalg.inv(a).T))
        models.append(m)
        corr.append(rng.permutation(len(w))[: len(w) * 2 // 3].astype(np.int64))
    return lists, models, corr
