"""One timepoint of the multiview pipeline, device resident (BASELINE configs[3]).

The Fiji workflow the reference runs per timepoint, restated over this library:

  1. Detect Interest Points   ProcessDOG.compute per view (spim/process/interestpointdetection/
                              ProcessDOG.java:40-178) -> bead positions in view pixels
  2. Register                 the view models are given; the correspondences the
                              registration would record are recovered from them (a detection
                              corresponds when another view detected a bead within ``radius``
                              world pixels of it).  With ``refine`` = "translation" / "rigid" /
                              "affine" the given models are first refined: pairwise matches
                              -> GlobalOpt.compute (globalopt.py, GlobalOpt.java:44-135),
                              view 0 fixed.  ``matching`` = "nearest" (the default) takes
                              mutual nearest detections within ``radius`` (the models must
                              already be right to that); "rgldm" runs the reference's
                              descriptor matching (RGLDMPairwise.java:34-77: candidates on
                              the GPU, RANSAC on the host; registration.py), which needs
                              only approximate models; "geometric_hashing" the rotation
                              invariant matcher (GeometricHashingPairwise.java:45-86), which
                              does not need their rotations either
  3. Input preparation        ProcessForDeconvolution.fuseStacksAndGetPSFs (:159-384): views
                              resampled into the bounding box, blending weights normalised,
                              and per view the PSF extracted from its corresponding beads
                              (getLocationsOfCorrespondingBeads :444-462, ExtractPSF.
                              extractNextImg :260-279) and transformed with the view model
  4. Deconvolution            MVDeconvolution (EfficientBayesianBased.java:166-286 defaults:
                              OPTIMIZATION_I, lambda 0.006)

Every volume stays in HBM (torch tensors are only device-memory plumbing); the
stages are the library's C-ABI calls.  ``process_timepoint`` returns psi as a
torch tensor and per-stage wall times.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass, field

import numpy as np

from . import _lib, dog, dom, input_prep, psf as psf_mod
from .decon import PSFTYPE, Session


@dataclass
class TimepointResult:
    psi: object                              # torch tensor [z, y, x] on the GPU
    points: list                             # per view: (n, 3) detections, view pixels (x, y, z)
    corresponding: list                      # per view: indices of detections with a correspondence
    psfs: list                               # per view: transformed PSF [z, y, x] (numpy)
    stats: np.ndarray                        # RL (iterations, views, 2)
    ms: dict = field(default_factory=dict)   # stage wall times
    engine: dict = field(default_factory=dict)   # RL FFT dims and z / x pass modes
    stage_digests: dict = field(default_factory=dict)   # SHA-256 per stage output (digest=True)
    models: list = field(default_factory=list)   # the view models used (refined when refine is set)
    globalopt: object = None                     # globalopt.GlobalOptResult (refine is set)
    bounding_box: tuple = None                   # (bb_min, bb_dims) used, (x, y, z) (estimated for bb_min="auto")
    reorientation: object = None                 # bb_min="reorient": the 3x4 transform preconcatenated to ``models``


def apply_model(model, pts):
    """AffineTransform3D.apply for (n, 3) points (x, y, z)."""
    m = np.asarray(model, np.float64).reshape(3, 4)
    return np.asarray(pts, np.float64) @ m[:, :3].T + m[:, 3]


def corresponding_detections(points, models, radius: float = 2.0, device=None):
    """The detections of each view that lie within ``radius`` world pixels of a
    detection of another view: the set ``getLocationsOfCorrespondingBeads`` reads
    from the registration's correspondence lists (ProcessForDeconvolution.java:444-462).

    All pairs within the radius are found exactly through a hash of radius-sized
    cells (sorted cell keys, the 27 neighbouring cells of each point looked up by
    binary search), in torch on ``device`` (the GPU in the pipeline, the CPU in
    the host tests)."""
    import torch
    dev = torch.device(device if device is not None else "cpu")
    world = [apply_model(m, p) if len(p) else np.zeros((0, 3)) for p, m in zip(points, models)]
    sizes = [len(w) for w in world]
    n = sum(sizes)
    if n == 0:
        return [np.zeros(0, np.int64) for _ in world]
    P = torch.from_numpy(np.concatenate(world)).to(dev, torch.float64)
    lab = torch.cat([torch.full((k,), v, dtype=torch.int64) for v, k in enumerate(sizes)]).to(dev)
    cell = torch.floor(P / radius).to(torch.int64)
    cell = cell - cell.min(dim=0).values + 1
    dims = cell.max(dim=0).values + 2
    key = (cell[:, 0] * dims[1] + cell[:, 1]) * dims[2] + cell[:, 2]
    skey, order = torch.sort(key)
    Ps, Ls = P[order], lab[order]
    r2 = float(radius) ** 2
    offs = torch.tensor([(dx * dims[1] + dy) * dims[2] + dz for dx in (-1, 0, 1) for dy in (-1, 0, 1)
                         for dz in (-1, 0, 1)], dtype=torch.int64, device=dev)
    nk = key[None, :] + offs[:, None]                          # [27, n] neighbouring cell keys
    lo = torch.searchsorted(skey, nk, side="left")
    cnt = torch.searchsorted(skey, nk, side="right") - lo
    hit = torch.zeros(n, dtype=torch.bool, device=dev)
    for j in range(int(cnt.max())):                            # (a cell rarely holds more than 2)
        idx = (lo + j).clamp(max=n - 1)
        d2 = ((Ps[idx] - P[None]) ** 2).sum(dim=2)
        hit |= ((j < cnt) & (Ls[idx] != lab[None]) & (d2 <= r2)).any(dim=0)
    hit = hit.cpu().numpy()
    out, o = [], 0
    for k in sizes:
        out.append(np.nonzero(hit[o:o + k])[0])
        o += k
    return out


def process_timepoint(views, models, bb_min, bb_dims=None, *, psf_size=(19, 19, 25), iterations: int = 10,
                      psftype: PSFTYPE = PSFTYPE.OPTIMIZATION_I, lam: float = 0.006, sigma: float = 1.8,
                      threshold: float = 0.008, localization: int = 1, radius: float = 2.0,
                      blending_border=(-8, -8, -8), blending_range=(12, 12, 12),
                      weight_type=input_prep.WeightType.VIRTUAL_WEIGHTS, device: int = 0,
                      log=None, digest: bool = False, refine: str | None = None,
                      dog_extension: str = "mirror", detector: str = "dog", radius1: int = 2,
                      radius2: int = 3, matching: str = "nearest", num_neighbors: int = 3,
                      redundancy: int = 1, ratio_of_distance: float | None = None,
                      difference_threshold: float = 50.0, max_epsilon: float = 5.0,
                      min_inlier_ratio: float = 0.1, min_inlier_factor: float = 3.0,
                      num_iterations: int = 1000, ransac_seed: int | None = None, icp: bool = False,
                      icp_max_distance: float = 5.0, icp_max_iterations: int = 100,
                      downsample_xy=1, downsample_z: int = 1, voxel_size=None,
                      max_detections: int | None = None,
                      max_detections_type: str = "brightest", auto_bb: dict | None = None,
                      reorient: dict | None = None, thin_out: dict | None = None) -> TimepointResult:
    """views: per view a [z, y, x] float32 torch tensor on the GPU (the acquired
    stack); models: 3x4 view -> world affines; bb_min / bb_dims (x, y, z), or bb_min="auto"
    (bb_dims None): the box is estimated from the views under the models the input preparation
    uses (``boundingbox.auto_bounding_box`` with the keywords of ``auto_bb``: background,
    discarded_object_size, downsampling), logged, recorded in ``bounding_box`` and timed as
    ``ms["auto_bounding_box"]``; ValueError when nothing is found; or bb_min="reorient" (bb_dims
    None): after the correspondences stage ``boundingbox.reorient_bounding_box`` finds, from
    ``points`` and -- unless ``reorient`` says ``corresponding=False`` -- only their corresponding
    detections (the dialog's default), the rotation under which the detections' box is smallest;
    the transform is preconcatenated to the models that input preparation and PSF extraction use
    (``models`` of the result), kept in ``reorientation``, the padded box (``reorient``:
    percent, default 10; reorientate) logged, recorded in ``bounding_box`` and timed as
    ``ms["reorient_bounding_box"]``;
    dog_extension: the detect stage's 'mirror' (accurate) or 'border' (approximate) GPU
    mode (``dog.compute``); detector: 'dog' (Difference-of-Gaussian: sigma) or 'dom'
    (Difference-of-Mean: radius1 / radius2, ``dom.compute``), both with threshold and
    localization; matching (used when ``refine`` is set): 'nearest', 'rgldm' with the
    RGLDM (num_neighbors, redundancy, ratio_of_distance, difference_threshold) and RANSAC
    (max_epsilon, min_inlier_ratio, min_inlier_factor, num_iterations, ransac_seed)
    parameters of ``registration.pairwise_rgldm``, or 'geometric_hashing' (rotation
    invariant: ratio_of_distance, difference_threshold and the RANSAC parameters of
    ``registration.pairwise_geometric_hashing``); ratio_of_distance None = the matcher's
    default, 3 for RGLDM and 10 for geometric hashing; icp (needs ``refine``): after that
    matching's global optimisation, ``registration.register_icp`` with model ``refine``,
    icp_max_distance and icp_max_iterations on the models it produced -- the reference's ICP
    run after a descriptor-based one; ``globalopt`` of the result then is the ICP run's;
    downsample_xy (1, 2, 4, 8, or 'match_z_less' / 'match_z_more', which need voxel_size
    (x, y, z)) and downsample_z: the detect stage runs on the downsampled views
    (``downsample.downsample``, DifferenceOf.openAndDownsample) and ``points`` are corrected to
    pixels of the full views, so every later stage is untouched; ``ms["downsample"]`` is that
    pass alone and is part of ``ms["detect"]``; max_detections / max_detections_type
    ('brightest', 'median', 'weakest'): ``downsample.limit_detections`` per view; thin_out (a
    dict with min_distance, max_distance and keep_range, by default 0, 5 and False):
    ``thinout.thin_out`` per view after that limit and before every later stage, in the units of
    voxel_size ((1, 1, 1) when that is None), the counts before and after logged per view
    (ThinOut_Detections.java:154-155); ``ms["thin_out"]`` is that step alone and is part of
    ``ms["detect"]``; None (the default): the step is not run."""
    import torch
    from . import downsample as ds
    ds_z = ds.downsample_factor(downsample_z)
    ds_xy = ds.downsample_factor(downsample_xy, ds_z, voxel_size)
    if max_detections_type not in ds.LIMIT_KINDS:
        raise ValueError(f"max_detections_type must be 'brightest', 'median' or 'weakest', not "
                         f"{max_detections_type!r}")
    to_kw = None
    if thin_out is not None:
        from . import thinout
        if not isinstance(thin_out, dict):
            raise ValueError("thin_out must be None or a dict with min_distance, max_distance and keep_range")
        unknown = sorted(set(thin_out) - {"min_distance", "max_distance", "keep_range"})
        if unknown:
            raise ValueError(f"thin_out: unknown keys {unknown}")
        to_range = float(thin_out.get("min_distance", 0.0)), float(thin_out.get("max_distance", 5.0))
        thinout.check_range(*to_range)
        to_voxel = (1.0, 1.0, 1.0) if voxel_size is None else tuple(float(x) for x in voxel_size)
        if len(to_voxel) != 3:
            raise ValueError("voxel_size must be (x, y, z)")
        to_kw = dict(voxel_size=to_voxel, min_distance=to_range[0], max_distance=to_range[1],
                     keep_range=bool(thin_out.get("keep_range", False)), device=device)
    if icp and refine is None:
        raise ValueError("icp=True needs refine (the model of the ICP registration)")
    if detector not in ("dog", "dom"):
        raise ValueError(f"detector must be 'dog' or 'dom', not {detector!r}")
    if matching not in ("nearest", "rgldm", "geometric_hashing"):
        raise ValueError(f"matching must be 'nearest', 'rgldm' or 'geometric_hashing', not {matching!r}")
    estimated = isinstance(bb_min, str)
    auto = estimated and bb_min == "auto"
    if estimated:
        if bb_min not in ("auto", "reorient"):
            raise ValueError(f"bb_min must be (x, y, z), 'auto' or 'reorient', not {bb_min!r}")
        if bb_dims is not None:
            raise ValueError(f"bb_min={bb_min!r} estimates bb_dims too: pass bb_dims=None")
        if (auto_bb is not None and not auto) or (reorient is not None and auto):
            raise ValueError("auto_bb goes with bb_min='auto', reorient with bb_min='reorient'")
    elif auto_bb is not None or reorient is not None or bb_dims is None:
        raise ValueError("an explicit bb_min needs bb_dims and no auto_bb / reorient (they go with bb_min='auto' / "
                         "'reorient')")
    ms = {}

    def lap(name, t0):
        torch.cuda.synchronize(device)
        ms[name] = round((time.perf_counter() - t0) * 1e3, 2)
        if log:
            log(f"{name}: {ms[name]} ms")
        return time.perf_counter()

    torch.cuda.synchronize(device)
    t = time.perf_counter()
    points = []
    t_ds = t_to = 0.0
    for v in views:          # 1. ProcessDOG (or ProcessDOM) per view, read in place
        if (ds_xy, ds_z) != (1, 1):   # (the call returns after its stream has drained)
            t0 = time.perf_counter()
            v = ds.downsample(v, ds_xy, ds_z, device=device)
            t_ds += time.perf_counter() - t0
        if detector == "dom":
            pos, inten = dom.interest_points_array(v, radius1=radius1, radius2=radius2, threshold=threshold,
                                                   localization=localization, device=device)
        else:
            pos, inten = dog.interest_points_array(v, sigma=sigma, threshold=threshold,
                                                   localization=localization, device=device,
                                                   extension=dog_extension)
        if (ds_xy, ds_z) != (1, 1):
            pos = ds.correct_for_downsampling(pos, ds_xy, ds_z)
        if max_detections is not None:
            pos, _ = ds.limit_detections(pos, inten, max_detections, max_detections_type)
            pos = np.ascontiguousarray(pos)
        if to_kw is not None:   # "Thin out detections", per view
            t0 = time.perf_counter()
            before = len(pos)
            pos = np.ascontiguousarray(thinout.thin_out(pos, **to_kw))
            t_to += time.perf_counter() - t0
            if log:
                log(f"thin out: view {len(points)}, detections: {before} >>> {len(pos)}")
        points.append(pos)
    if (ds_xy, ds_z) != (1, 1):
        ms["downsample"] = round(t_ds * 1e3, 2)
    if to_kw is not None:
        ms["thin_out"] = round(t_to * 1e3, 2)
    t = lap("detect", t)
    gres = None
    models = [np.asarray(m, np.float64).reshape(3, 4) for m in models]
    if refine is not None:   # 2'. GlobalOpt over pairwise matches (host)
        from . import globalopt
        if matching == "rgldm":   # RGLDM candidates on the views' device, RANSAC on the host
            from . import registration
            seed = registration.RANSAC_SEED if ransac_seed is None else ransac_seed
            matches = registration.pairwise_rgldm(
                points, models, model=refine, num_neighbors=num_neighbors, redundancy=redundancy,
                ratio_of_distance=3.0 if ratio_of_distance is None else ratio_of_distance,
                difference_threshold=difference_threshold,
                max_epsilon=max_epsilon, min_inlier_ratio=min_inlier_ratio, min_inlier_factor=min_inlier_factor,
                num_iterations=num_iterations, seed=seed, device=device)
        elif matching == "geometric_hashing":   # rotation invariant candidates, the same host RANSAC
            from . import registration
            seed = registration.RANSAC_SEED if ransac_seed is None else ransac_seed
            matches = registration.pairwise_geometric_hashing(
                points, models, model=refine,
                ratio_of_distance=10.0 if ratio_of_distance is None else ratio_of_distance,
                difference_threshold=difference_threshold,
                max_epsilon=max_epsilon, min_inlier_ratio=min_inlier_ratio, min_inlier_factor=min_inlier_factor,
                num_iterations=num_iterations, seed=seed, device=device)
        else:
            matches = globalopt.correspondences(points, models, radius)
        gres = globalopt.compute(len(models), matches, model=refine, fixed=(0,))
        if gres is not None:   # (a caught fit failure keeps the tiles' models as they stand, as the reference)
            if gres.failure and log:
                log(gres.failure)
            models = [globalopt.concatenate(c, m) for c, m in zip(gres.models, models)]
        if icp:   # every detection re-matched under the models so far (assignment on the views' device)
            from . import registration
            models, gres = registration.register_icp(points, models, model=refine, fixed=(0,),
                                                     max_distance=icp_max_distance,
                                                     max_iterations=icp_max_iterations, device=device)
            if gres is not None and gres.failure and log:
                log(gres.failure)
        t = lap("register", t)
    corr = corresponding_detections(points, models, radius, device=f"cuda:{device}")   # 2. (registration given)
    t = lap("correspondences", t)
    if auto:   # 2b. "Estimate automatically": the box from the data, under the models used below
        from . import boundingbox
        bb_min, bb_dims = boundingbox.auto_bounding_box(list(views), models, device=device, **(auto_bb or {}))
        if log:
            log(f"automatic bounding box: min {bb_min}, dims {bb_dims}")
        t = lap("auto_bounding_box", t)
    reorientation = None
    if estimated and not auto:   # 2c. "Automatically reorientate and estimate based on sample features"
        from . import boundingbox
        ro = dict(reorient or {})
        use_corr = ro.pop("corresponding", True)
        reorientation, models, bb_min, bb_dims = boundingbox.reorient_bounding_box(
            points, models, corresponding=corr if use_corr else None, device=device, **ro)
        if log:
            log(f"reorienting bounding box: min {bb_min}, dims {bb_dims}, transform "
                f"{[round(float(x), 6) for x in reorientation.reshape(12)]}")
        t = lap("reorient_bounding_box", t)
    imgs, ws, info = input_prep.prepare_inputs(views, models, bb_min, bb_dims, blending_border, blending_range,
                                               weight_type, device=device)   # 3a.
    t = lap("prepare_inputs", t)
    # 3b. ExtractPSF from the corresponding beads, all views at once (a view with no
    # corresponding bead -- registration would have failed for it -- takes all of its
    # detections rather than an all-zero PSF)
    beads = [p[c] if len(c) else p for p, c in zip(points, corr)]
    psfs = [tr for _, tr in psf_mod.extract_psfs(list(views), beads, psf_size, list(models), device=device)]
    psf_mod.release_workspace(device)   # (the bead samples and per-view buffers: HBM the RL session can use)
    t = lap("extract_psf", t)
    sd = {}
    if digest:   # (outside the timed stages' accounting: after the lap)
        # one volume on the host at a time (a C4 timepoint is 16 volumes of 768^3 float32)
        sd["inputs"] = _sha(x.cpu().numpy() for x in list(imgs) + list(ws))
        sd["psfs"] = _sha(np.ascontiguousarray(p, np.float32) for p in psfs)
        sd["corresponding"] = _sha(np.ascontiguousarray(c, np.int64) for c in corr)
        t = time.perf_counter()
    shape = tuple(imgs[0].shape)
    t_setup = t
    sess = Session((shape[2], shape[1], shape[0]), device=device)            # 4. MVDeconvolution
    try:
        t = lap("rl_setup_create", t)
        for i, w, k in zip(imgs, ws, psfs):
            sess.add_view_device(i.data_ptr(), w.data_ptr(), k)
        t = lap("rl_setup_add_views", t)
        sess.init(psftype)
        sess.init_psi()
        engine = {"fft_dims_xyz": list(sess.fft_dims(0)), "zpass_mode": sess.zpass_mode(0),
                  "kernel_planes": sess.kernel_planes(0)}
        t = lap("rl_setup_init", t)
        ms["rl_setup"] = round((t - t_setup) * 1e3, 2)
        stats = sess.run(iterations, lam)
        engine["xpass_mode"] = sess.xpass_mode(0)
        sess.apply_mask()
        t = lap("rl_iterations", t)
        psi = torch.empty(shape, dtype=torch.float32, device=imgs[0].device)
        _lib.check(sess.lib.mvd_get_psi(sess.h, C.cast(C.c_void_p(psi.data_ptr()), _lib._pf)))
    finally:
        sess.close()
    del imgs, ws
    lap("rl_result", t)
    return TimepointResult(psi, points, corr, psfs, stats, ms, engine, sd, models, gres,
                           (tuple(int(x) for x in bb_min), tuple(int(x) for x in bb_dims)), reorientation)


def _sha(parts) -> str:
    """SHA-256 of the concatenated bytes of `parts` (arrays), fed one part at a time."""
    import hashlib
    h = hashlib.sha256()
    for a in parts:
        h.update(memoryview(np.ascontiguousarray(a)).cast("B"))
    return h.hexdigest()


class Pipeline:
    """The per-timepoint driver held across a time series (BASELINE configs[3]): the
    parameters of every stage, and the device whose library-side state (the DoG
    workspace, the PSF / resampling scratch, plan caches) carries over from one
    timepoint to the next -- as the reference's plugin processes timepoint after
    timepoint (EfficientBayesianBased.java:166-286).  Carried state must not change a
    result: timepoint t processed after others equals timepoint t processed alone
    (``result_digest``; tests/test_gpu_scale.py)."""

    def __init__(self, **params):
        self.params = params

    def process(self, views, models, bb_min, bb_dims=None, log=None, digest=False) -> TimepointResult:
        return process_timepoint(views, models, bb_min, bb_dims, log=log, digest=digest, **self.params)


def result_digest(res: TimepointResult) -> dict:
    """SHA-256 of psi's bytes and of the RL statistics, plus the detection counts."""
    import hashlib
    psi = res.psi.cpu().numpy()
    return {**{f"{k}_sha256": v for k, v in res.stage_digests.items()},
            "psi_sha256": hashlib.sha256(psi.tobytes()).hexdigest(),
            "stats_sha256": hashlib.sha256(np.ascontiguousarray(res.stats, np.float64).tobytes()).hexdigest(),
            "points_sha256": hashlib.sha256(b"".join(np.ascontiguousarray(p, np.float64).tobytes()
                                                     for p in res.points)).hexdigest()}
