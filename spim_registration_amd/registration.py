"""Descriptor-based pairwise registration: RGLDM candidates on the GPU, RANSAC and the
global optimisation on the host.

The reference's default matcher when only detections and approximate view models are known
is the "redundant geometric local descriptor matching" (translation invariant):

  spim/process/interestpointregistration/geometricdescriptor/RGLDMPairwise.java:34-77
  .../geometricdescriptor/RGLDMMatcher.java:44-123, RGLDMParameters.java (3 / 1 / 3 / 50)
  mpicbg/pointdescriptor/{AbstractPointDescriptor,SimplePointDescriptor}.java,
  matcher/SubsetMatcher.java, similarity/SquareDistance.java

Every point is described by the vectors to its ``num_neighbors + redundancy`` nearest
neighbours; two descriptors are compared over every pair of ``num_neighbors``-subsets, and a
point of A is a candidate when its best B descriptor is below ``difference_threshold`` and
``ratio_of_distance`` times better than the second best.  ``rgldm_candidates`` /
``descriptors`` run that on the GPU (``spim_rgldm_match`` / ``spim_rgldm_descriptors``,
csrc/rgldm.hip), bit-exact against the reference's arithmetic; there is no CPU path.  The
order of neighbours at exactly the same float distance is unpinned (lower index first here;
the reference's fiji.util.KDTree is not in its tree).

RGLDM is translation invariant only.  The reference's "fast 3d geometric hashing (rotation
invariant)" (geometrichashing/GeometricHashingPairwise.java:45-86, GeometricHasher.java:54-116,
mpicbg/pointdescriptor/LocalCoordinateSystemPointDescriptor.java) describes a point by its 3
nearest neighbours in their own local coordinate system -- six floats -- and takes an A point as
a candidate when its best B descriptor is below ``difference_threshold`` (50) and its distance
times ``ratio_of_distance`` (10) not above the second best's.  ``gh_candidates`` /
``gh_descriptors`` run that on the GPU (``spim_gh_match`` / ``spim_gh_descriptors``,
csrc/geohash.hip), bit-exact too; unpinned is the ranking of B descriptors (by the float root
of the distance, lower index first on equal floats, NaN not ranked).

``ransac`` restates ``RANSAC.computeRANSAC`` (spim/process/interestpointregistration/
RANSAC.java:21-110) over mpicbg's ``Model.filterRansac`` on the host, in NumPy, with the
model fits of ``globalopt.fit``.  Parity unpinned: mpicbg is not in the reference tree, so
``filterRansac`` is restated from its published algorithm --

  * ransac: ``num_iterations`` times draw a minimal sample of distinct candidates (index
    ``int(u * n)``, redrawn while already chosen), fit, take the candidates closer than
    ``max_epsilon`` as inliers, and refit on them while their number grows; a hypothesis is
    good when it has at least the model's minimum of inliers and an inlier ratio above
    ``min_inlier_ratio``; the good hypothesis with the strictly largest ratio is kept
  * filter (maxTrust 4): refit on the kept set, drop matches farther than 4 x the median
    distance, until none is dropped; the cost is the mean distance of the last fit

-- and its random draws cannot match Java's.  The generator is NumPy's
``Generator(PCG64(seed))`` and ``u = generator.random()``; the result is deterministic for a
given seed.  Regularised models (``InterpolatedAffineModel3D``) are out of scope: ``model``
is "translation", "rigid" or "affine".  RANSAC stays on the host on purpose: 10^3
hypotheses over a few thousand candidates take milliseconds.

The reference's third matcher, "Iterative closest-point (ICP, no invariance)"
(icp/IterativeClosestPointPairwise.java:40-122, mpicbg/icp/ICP.java:91-115 and :208-317,
SimplePointMatchIdentification.java:32-48), is a registration run of its own after a descriptor
one: it re-matches every detection under the current model, which multiplies the
correspondences.  ``icp_assign`` runs one iteration's search on the GPU (``spim_icp_assign``,
csrc/icp.hip: the model applied to the target list, per reference point the nearest target by
``Detection.distanceTo``, the threshold, ambiguous matches removed), bit-exact; ``icp`` is the
loop with the fits of ``globalopt.fit``, ``pairwise_icp`` / ``register_icp`` the entry points.
Unpinned: the order among equal float distances (lower target index first; the reference's
kd-tree is not in its tree) and mpicbg's ``fit`` / ``apply`` (restated in ``globalopt``).
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib, globalopt
from ._lib import check

__all__ = ["rgldm_candidates", "descriptors", "ransac", "pairwise_rgldm", "register", "tile_sizes",
           "gh_candidates", "gh_descriptors", "gh_tile_sizes", "pairwise_geometric_hashing",
           "icp_tile_sizes", "icp_assign", "icp", "pairwise_icp", "register_icp"]

RANSAC_SEED = 4711


def _params(lib, num_neighbors, redundancy, ratio_of_distance, difference_threshold, device, b_split=0):
    p = _lib.RgldmParams()
    lib.spim_rgldm_params_default(C.byref(p))
    p.num_neighbors, p.redundancy = int(num_neighbors), int(redundancy)
    p.ratio_of_distance, p.difference_threshold = float(ratio_of_distance), float(difference_threshold)
    p.b_split, p.device = int(b_split), int(device)
    return p


def _points(x):
    """(pointer, n, the object that owns the memory) of an (n, 3) double array: a numpy array
    or a CUDA torch tensor (read in place)."""
    if hasattr(x, "is_cuda") and x.is_cuda:
        import torch
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError("points must be (n, 3)")
        x = x.contiguous().double()
        torch.cuda.synchronize(x.device)   # the library runs on its own stream
        return C.c_void_p(x.data_ptr()), int(x.shape[0]), x
    a = np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1, 3))
    return C.c_void_p(a.ctypes.data), len(a), a


def _tiles(fn):
    a, b = C.c_int32(0), C.c_int32(0)
    fn(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def _candidates(fn, params, pa, pb, return_all):
    """a candidate matcher's call (``spim_rgldm_match`` / ``spim_gh_match``) and its results"""
    aptr, na, _ka = _points(pa)
    bptr, nb, _kb = _points(pb)
    idx, best, second = np.empty(na, np.int32), np.empty(na, np.float64), np.empty(na, np.float64)
    ia, ib = np.empty(max(na, 1), np.int32), np.empty(max(na, 1), np.int32)   # at most one candidate per A point
    n = C.c_int64(0)
    check(fn(aptr, na, bptr, nb, C.byref(params), C.c_void_p(idx.ctypes.data), C.c_void_p(best.ctypes.data),
             C.c_void_p(second.ctypes.data), C.c_void_p(ia.ctypes.data), C.c_void_p(ib.ctypes.data), na, C.byref(n)))
    ia, ib = ia[:n.value].copy(), ib[:n.value].copy()
    return (ia, ib, idx, best, second) if return_all else (ia, ib)


def tile_sizes():
    """(A descriptors per block, B descriptors per LDS tile) of the matching kernel."""
    return _tiles(_lib.load().spim_rgldm_tiles)


def descriptors(points, num_neighbors: int = 3, redundancy: int = 1, device: int = 0):
    """createSimplePointDescriptors: (neighbors (n, nn+re) int32 -- the nearest other points
    in ascending float distance --, rel (n, nn+re, 3) float64 -- neighbour minus basis)."""
    lib = _lib.load()
    p = _params(lib, num_neighbors, redundancy, 3.0, 50.0, device)
    ptr, n, _keep = _points(points)
    m = max(int(num_neighbors) + int(redundancy), 0)
    nbr = np.empty((n, m), np.int32)
    rel = np.empty((n, m, 3), np.float64)
    check(lib.spim_rgldm_descriptors(ptr, n, C.byref(p), C.c_void_p(nbr.ctypes.data), C.c_void_p(rel.ctypes.data)))
    return nbr, rel


def rgldm_candidates(pa, pb, num_neighbors: int = 3, redundancy: int = 1, ratio_of_distance: float = 3.0,
                     difference_threshold: float = 50.0, device: int = 0, return_all: bool = False,
                     b_split: int = 0):
    """RGLDMMatcher.extractCorrespondenceCandidates over two (n, 3) point lists (numpy arrays
    or CUDA torch tensors, x, y, z in one common frame): (ia, ib), candidate k pairs
    pa[ia[k]] with pb[ib[k]], in ascending ia; with ``return_all`` also best_idx, best and
    second over every point of pa.  ``b_split`` forces the partitions of B (0 = auto; the
    result does not depend on it)."""
    lib = _lib.load()
    p = _params(lib, num_neighbors, redundancy, ratio_of_distance, difference_threshold, device, b_split)
    return _candidates(lib.spim_rgldm_match, p, pa, pb, return_all)


def _gh_params(lib, ratio_of_distance, difference_threshold, device, b_split=0):
    p = _lib.GhParams()
    lib.spim_gh_params_default(C.byref(p))
    p.ratio_of_distance, p.difference_threshold = float(ratio_of_distance), float(difference_threshold)
    p.b_split, p.device = int(b_split), int(device)
    return p


def gh_tile_sizes():
    """(A descriptors per block, B descriptors per LDS tile) of the geometric hashing
    matching kernel."""
    return _tiles(_lib.load().spim_gh_tiles)


def gh_descriptors(points, device: int = 0):
    """createLocalCoordinateSystemPointDescriptors (GeometricHasher.java:87-116) of at least
    4 points: (neighbors (n, 3) int32 -- the nearest other points in ascending float distance
    --, desc (n, 6) float32 -- ax bx by cx cy cz of LocalCoordinateSystemPointDescriptor)."""
    lib = _lib.load()
    p = _gh_params(lib, 10.0, 50.0, device)
    ptr, n, _keep = _points(points)
    nbr = np.empty((n, 3), np.int32)
    desc = np.empty((n, 6), np.float32)
    check(lib.spim_gh_descriptors(ptr, n, C.byref(p), C.c_void_p(nbr.ctypes.data), C.c_void_p(desc.ctypes.data)))
    return nbr, desc


def gh_candidates(pa, pb, ratio_of_distance: float = 10.0, difference_threshold: float = 50.0, device: int = 0,
                  return_all: bool = False, b_split: int = 0):
    """GeometricHasher.extractCorrespondenceCandidates (rotation invariant) over two (n, 3)
    point lists (numpy arrays or CUDA torch tensors, x, y, z): (ia, ib), candidate k pairs
    pa[ia[k]] with pb[ib[k]], in ascending ia; with ``return_all`` also best_idx, best and
    second over every point of pa.  Fewer than 4 points in either list: no candidates.
    ``b_split`` forces the partitions of B (0 = auto; the result does not depend on it)."""
    lib = _lib.load()
    p = _gh_params(lib, ratio_of_distance, difference_threshold, device, b_split)
    return _candidates(lib.spim_gh_match, p, pa, pb, return_all)


def icp_tile_sizes():
    """(reference points per block, target points per LDS tile) of the ICP assignment kernel."""
    return _tiles(_lib.load().spim_icp_tiles)


def icp_assign(target, reference, model=None, max_distance: float = 5.0, device: int = 0, return_all: bool = False,
               t_split: int = 0):
    """One ICP iteration up to the fit (ICP.runICPIteration, ICP.java:91-101) over two (n, 3)
    point lists (numpy arrays or CUDA torch tensors): the target moved by the 3x4 ``model``
    (None = the identity), per reference point its nearest target by ``Detection.distanceTo``
    (lower index among equal floats), a match when that float distance is <=
    ``(float) max_distance``, and the matches that share a target removed.  Returns (it, ir),
    match k pairs target[it[k]] with reference[ir[k]], in ascending ir; with ``return_all`` also
    nearest (int32) and dist (float32) over every reference point and the number of ambiguous
    matches removed.  ``t_split`` forces the partitions of the target (0 = auto; the result
    does not depend on it)."""
    lib = _lib.load()
    p = _lib.IcpParams()
    lib.spim_icp_params_default(C.byref(p))
    p.max_distance, p.t_split, p.device = float(max_distance), int(t_split), int(device)
    tptr, nt, _kt = _points(target)
    rptr, nr, _kr = _points(reference)
    m = None if model is None else np.ascontiguousarray(np.asarray(model, np.float64).reshape(12))
    nearest, dist = np.empty(nr, np.int32), np.empty(nr, np.float32)
    it, ir = np.empty(max(nr, 1), np.int32), np.empty(max(nr, 1), np.int32)   # at most one match per reference point
    n, amb = C.c_int64(0), C.c_int64(0)
    check(lib.spim_icp_assign(tptr, nt, rptr, nr, None if m is None else C.c_void_p(m.ctypes.data), C.byref(p),
                              C.c_void_p(nearest.ctypes.data), C.c_void_p(dist.ctypes.data),
                              C.c_void_p(it.ctypes.data), C.c_void_p(ir.ctypes.data), nr, C.byref(n), C.byref(amb)))
    it, ir = it[:n.value].copy(), ir[:n.value].copy()
    return (it, ir, nearest, dist, int(amb.value)) if return_all else (it, ir)


def icp(pa, pb, model: str = "affine", max_distance: float = 5.0, max_iterations: int = 100, device: int = 0,
        assign=None):
    """IterativeClosestPointPairwise.call (:40-122) over the target list ``pa`` and the reference
    list ``pb`` ((n, 3), one common frame): from the identity, assign (``icp_assign`` on GPU
    ``device``) under the current model, fit ``model`` to the matches (``globalopt.fit``, pa ->
    pb; the model is absolute, not incremental), until an iteration's number of matches and mean
    error both equal the previous one's, ``max_iterations`` at the most.  Returns (it, ir, the
    3x4 model, the mean error of the matches under it, the reference's iteration count ``i``);
    fewer points than the model's minimum in a list, or a fit that fails
    (NotEnoughDataPoints, IllDefinedDataPoints): ((0,) indices twice, None, NaN, i).  The lists
    are uploaded once; the errors are NumPy's on the host.  ``assign``: a callable with
    ``icp_assign``'s signature to use in place of the GPU (the tests feed the restatement
    through the same loop)."""
    if model not in globalopt.MIN_MATCHES:
        raise ValueError(f"model must be one of {sorted(globalopt.MIN_MATCHES)}")
    pa = np.ascontiguousarray(np.asarray(pa, np.float64).reshape(-1, 3))
    pb = np.ascontiguousarray(np.asarray(pb, np.float64).reshape(-1, 3))
    empty = np.zeros(0, np.int32)
    least = globalopt.MIN_MATCHES[model]
    if len(pa) < least or len(pb) < least:   # "Not enough detections to match"
        return empty, empty, None, float("nan"), 0
    if assign is None:
        import torch
        ta, tb = (torch.tensor(x, dtype=torch.float64, device=f"cuda:{int(device)}") for x in (pa, pb))
        kw = dict(max_distance=max_distance, device=device)
        assign = icp_assign
    else:
        ta, tb = pa, pb
        kw = dict(max_distance=max_distance)
    m = np.hstack([np.eye(3), np.zeros((3, 1))])
    i, last_n, last_err = 0, 0, 0.0
    while True:
        it, ir = assign(ta, tb, model=m, **kw)
        try:
            m = globalopt.fit(model, pa[it], pb[ir], np.ones(len(it)))
        except (globalopt.NotEnoughDataPoints, globalopt.IllDefinedDataPoints):
            return empty, empty, None, float("nan"), i
        err = float(np.linalg.norm(globalopt.apply(m, pa[it]) - pb[ir], axis=1).mean())   # PointMatch.meanDistance
        converged = last_n == len(it) and last_err == err
        last_n, last_err = len(it), err
        if converged:
            break
        i += 1
        if not i < int(max_iterations):
            break
    return it, ir, m, err, i


def _world_and_pairs(points, models, pairs):
    """(the views' detections mapped by their current models, the given pairs or all of them)"""
    world = [globalopt.apply(np.asarray(m, np.float64).reshape(3, 4), np.asarray(p, np.float64).reshape(-1, 3))
             for p, m in zip(points, models)]
    if pairs is None:
        pairs = [(a, b) for a in range(len(world)) for b in range(a + 1, len(world))]
    return world, pairs


def _refine(models, matches, model, fixed):
    """``globalopt.compute`` over the pairwise matches and ``globalopt.concatenate`` onto the
    given 3x4 models: (the refined models -- the given ones when no pair has matches --, the
    GlobalOptResult or None)"""
    res = globalopt.compute(len(models), matches, model=model, fixed=fixed)
    if res is not None:
        models = [globalopt.concatenate(c, m) for c, m in zip(res.models, models)]
    return models, res


def pairwise_icp(points, models, pairs=None, model: str = "affine", max_distance: float = 5.0,
                 max_iterations: int = 100, device: int = 0, assign=None):
    """IterativeClosestPointPairwise.call over all view pairs (or ``pairs``, (a, b) tuples): the
    views' detections mapped by their current ``models``, view a the target and view b the
    reference of ``icp``.  Returns the pairs with matches as ``globalopt.PairwiseMatch`` over
    world points under ``models`` (the last iteration's matches are candidates and inliers
    alike; the pair's model is not passed on, the global optimisation refits)."""
    world, pairs = _world_and_pairs(points, models, pairs)
    out = []
    for a, b in pairs:
        it, ir, _, _, _ = icp(world[a], world[b], model, max_distance, max_iterations, device, assign)
        if len(it):
            out.append(globalopt.PairwiseMatch(a, b, world[a][it], world[b][ir]))
    return out


def register_icp(points, models, model: str = "affine", fixed=(0,), **kw):
    """ICP registration of the views from their detections and models that are already close
    (the reference runs it after a descriptor-based registration): ``pairwise_icp`` (its
    keywords pass through), ``globalopt.compute`` and ``globalopt.concatenate``.  Returns what
    ``register`` returns."""
    models = [np.asarray(m, np.float64).reshape(3, 4) for m in models]
    return _refine(models, pairwise_icp(points, models, model=model, **kw), model, fixed)


def _inliers(kind, pa, pb, sel, eps):
    """(model fitted to the matches sel, the candidates closer than eps under it)"""
    m = globalopt.fit(kind, pa[sel], pb[sel], np.ones(len(sel)))
    d = np.linalg.norm(globalopt.apply(m, pa) - pb, axis=1)
    return m, np.nonzero(d < eps)[0]


def ransac(pa, pb, model: str = "affine", max_epsilon: float = 5.0, min_inlier_ratio: float = 0.1,
           min_inlier_factor: float = 3.0, num_iterations: int = 1000, seed: int = RANSAC_SEED):
    """RANSAC.computeRANSAC over the candidates pa[i] <-> pb[i]: (inlier indices, the 3x4
    model pa -> pb refitted on them, its mean error ``model.getCost()``); with too few
    candidates, no model or too few inliers ((0,) indices, None, NaN)."""
    if model not in globalopt.MIN_MATCHES:
        raise ValueError(f"model must be one of {sorted(globalopt.MIN_MATCHES)}")
    pa = np.asarray(pa, np.float64).reshape(-1, 3)
    pb = np.asarray(pb, np.float64).reshape(-1, 3)
    if len(pa) != len(pb):
        raise ValueError("ransac needs as many points in pa as in pb")
    none = (np.zeros(0, np.int64), None, float("nan"))
    n, least = len(pa), globalopt.MIN_MATCHES[model]
    # Math.round = floor(x + 0.5) (RANSAC.java:31)
    min_num = max(least, int(np.floor(least * float(min_inlier_factor) + 0.5)))
    if n < min_num:
        return none
    rng = np.random.Generator(np.random.PCG64(seed))
    best_set, best_ratio = None, 0.0
    for _ in range(int(num_iterations)):
        sample = []
        while len(sample) < least:
            j = int(rng.random() * n)
            if j not in sample:
                sample.append(j)
        try:
            _, inl = _inliers(model, pa, pb, np.asarray(sample), max_epsilon)
            good = len(inl) >= least and len(inl) / n > min_inlier_ratio
            grown = 0
            while good and grown < len(inl):
                grown = len(inl)
                _, inl = _inliers(model, pa, pb, inl, max_epsilon)
                good = len(inl) >= least and len(inl) / n > min_inlier_ratio
        except globalopt.IllDefinedDataPoints:
            continue
        if good and len(inl) / n > best_ratio:
            best_set, best_ratio = inl, len(inl) / n
    if best_set is None:
        return none
    # Model.filter, maxTrust 4: the median-based filter
    inl = best_set
    while True:
        try:
            m = globalopt.fit(model, pa[inl], pb[inl], np.ones(len(inl)))
        except (globalopt.NotEnoughDataPoints, globalopt.IllDefinedDataPoints):
            return none
        d = np.linalg.norm(globalopt.apply(m, pa[inl]) - pb[inl], axis=1)
        cost = float(d.mean())
        kept = inl[d <= float(np.median(d)) * 4.0]
        if len(kept) == len(inl):
            break
        inl = kept
    if len(inl) < max(least, min_num):
        return none
    return inl, m, cost


def _pairwise_ransac(world, pairs, find, model, max_epsilon, min_inlier_ratio, min_inlier_factor, num_iterations,
                     seed):
    """per pair the candidates ``find(pa, pb) -> (ia, ib)`` through ``ransac``: the pairs with
    inliers as ``globalopt.PairwiseMatch``"""
    out = []
    for a, b in pairs:
        ia, ib = find(world[a], world[b])
        ca, cb = world[a][ia], world[b][ib]
        inl, _, _ = ransac(ca, cb, model, max_epsilon, min_inlier_ratio, min_inlier_factor, num_iterations, seed)
        if len(inl):
            out.append(globalopt.PairwiseMatch(a, b, ca[inl], cb[inl]))
    return out


def pairwise_rgldm(points, models, pairs=None, model: str = "affine", num_neighbors: int = 3, redundancy: int = 1,
                   ratio_of_distance: float = 3.0, difference_threshold: float = 50.0, max_epsilon: float = 5.0,
                   min_inlier_ratio: float = 0.1, min_inlier_factor: float = 3.0, num_iterations: int = 1000,
                   seed: int = RANSAC_SEED, device: int = 0, candidates=None):
    """RGLDMPairwise.call over all view pairs (or ``pairs``, (a, b) tuples): the views'
    detections mapped by their current ``models`` (GlobalOptimizationType.java:208-213), the
    RGLDM candidates on GPU ``device``, RANSAC on the host.  Returns the pairs with inliers
    as ``globalopt.PairwiseMatch`` over world points under ``models``.  ``candidates``: a
    callable (pa, pb, **rgldm parameters) -> (ia, ib) to use in place of the GPU matcher
    (the tests feed the restatement's candidates through the same code)."""
    world, pairs = _world_and_pairs(points, models, pairs)
    kw = dict(num_neighbors=num_neighbors, redundancy=redundancy, ratio_of_distance=ratio_of_distance,
              difference_threshold=difference_threshold)
    if candidates is None:
        candidates = functools.partial(rgldm_candidates, device=device)
    return _pairwise_ransac(world, pairs, functools.partial(candidates, **kw), model, max_epsilon, min_inlier_ratio,
                            min_inlier_factor, num_iterations, seed)


def pairwise_geometric_hashing(points, models, pairs=None, model: str = "affine", ratio_of_distance: float = 10.0,
                               difference_threshold: float = 50.0, max_epsilon: float = 5.0,
                               min_inlier_ratio: float = 0.1, min_inlier_factor: float = 3.0,
                               num_iterations: int = 1000, seed: int = RANSAC_SEED, device: int = 0,
                               candidates=None):
    """GeometricHashingPairwise.call (:45-86) over all view pairs (or ``pairs``): as
    ``pairwise_rgldm`` with the rotation invariant geometric hashing candidates
    (``gh_candidates``) in place of RGLDM's, so the ``models`` need not be rotationally
    right.  ``candidates``: a callable (pa, pb, ratio_of_distance=, difference_threshold=)
    -> (ia, ib) to use in place of the GPU matcher."""
    world, pairs = _world_and_pairs(points, models, pairs)
    kw = dict(ratio_of_distance=ratio_of_distance, difference_threshold=difference_threshold)
    if candidates is None:
        candidates = functools.partial(gh_candidates, device=device)
    return _pairwise_ransac(world, pairs, functools.partial(candidates, **kw), model, max_epsilon, min_inlier_ratio,
                            min_inlier_factor, num_iterations, seed)


def register(points, models, model: str = "affine", fixed=(0,), matching: str = "rgldm", **kw):
    """Descriptor-based registration of the views from their detections and approximate
    models: ``pairwise_rgldm`` -- or, with ``matching`` = "geometric_hashing",
    ``pairwise_geometric_hashing`` -- (its keywords pass through), ``globalopt.compute`` and
    ``globalopt.concatenate``.  Returns (the refined 3x4 models, the GlobalOptResult -- None
    when no pair has inliers, the models then are the given ones)."""
    if matching not in ("rgldm", "geometric_hashing"):
        raise ValueError(f"matching must be 'rgldm' or 'geometric_hashing', not {matching!r}")
    models = [np.asarray(m, np.float64).reshape(3, 4) for m in models]
    pairwise = pairwise_rgldm if matching == "rgldm" else pairwise_geometric_hashing
    return _refine(models, pairwise(points, models, model=model, **kw), model, fixed)
