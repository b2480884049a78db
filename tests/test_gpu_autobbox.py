"""GPU: the automatic bounding box (csrc/autobbox.hip through boundingbox.py) bit for bit
against the restatement tests/autobbox_ref.py.  Floats are compared through their uint32 view,
so that -0 and NaN count."""
import ctypes as C

import numpy as np
import pytest

import autobbox_ref as ar
from spim_registration_amd import _lib, boundingbox as bb

pytestmark = pytest.mark.gpu


def u32(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_image(shape, seed):
    """[-1, 1]: the zero extension bites where the face is positive and not where it is negative"""
    return (np.random.default_rng(seed).random(shape) * 2 - 1).astype(np.float32)


def special_image():
    """one NaN voxel, and a patch of -0.0 beside +0.0 in an otherwise positive region"""
    img = random_image((9, 31, 257), 5)
    img[:, 6:22, 100:180] = np.abs(img[:, 6:22, 100:180]) + 0.5
    img[4, 12:15, 130:140] = 0.0
    img[4, 13, 133:137] = -0.0
    img[7, 25, 200] = np.nan
    return img


# [z, y, x], radius: the smallest shapes at which the tiling can go wrong
FILTER_CASES = [
    ((1, 1, 1), 1),            # a single voxel
    ((3, 5, 7), 50),           # every axis shorter than the window
    ((9, 31, 257), 1),         # x beyond a tile, odd sizes
    ((9, 31, 257), 3),
    ((70, 45, 130), 12),       # windows crossing tile seams on all three axes
    ((5, 200, 66), 64),        # the largest supported radius
    ((3, 5, 67), 2),           # no extent a multiple of any tile, narrower than the halo along z
]


@pytest.fixture(scope="module")
def filter_refs():
    """per case (image, restated filter), computed once and never written to"""
    refs = {}
    for i, (shape, r) in enumerate(FILTER_CASES):
        img = random_image(shape, 100 + i)
        refs[(shape, r)] = (img, ar.min_filter(img, r))
    sp = special_image()
    refs["special"] = (sp, ar.min_filter(sp, 3))
    for v in refs.values():
        for a in v:
            a.setflags(write=False)
    return refs


def staged(img, on_device):
    """a private copy of img where the call shall find it, and its address"""
    import torch
    a = torch.from_numpy(img.copy()).cuda() if on_device else img.copy()
    torch.cuda.synchronize()   # the library runs on its own stream
    return a, C.c_void_p(a.data_ptr() if on_device else a.ctypes.data)


def dims_of(img):
    return (C.c_int64 * 3)(*img.shape[::-1])


@pytest.mark.parametrize("shape,r", FILTER_CASES)
def test_min_filter_host_and_device(gpu, lib, filter_refs, shape, r):
    import torch
    img, want = filter_refs[(shape, r)]
    # the C entry with every pairing of a host / device-resident image and result
    for src_dev in (False, True):
        for out_dev in (False, True):
            src, sp = staged(img, src_dev)
            out, op = staged(np.zeros_like(img), out_dev)
            assert lib.spim_min_filter(sp, dims_of(img), r, 0, op) == 0
            np.testing.assert_array_equal(u32(out), u32(want), err_msg=f"{src_dev} {out_dev}")
            np.testing.assert_array_equal(u32(src), u32(img))       # the input is only read
    got = bb.min_filter(img, r)
    assert isinstance(got, np.ndarray) and got.shape == img.shape
    np.testing.assert_array_equal(u32(got), u32(want))
    dimg = torch.from_numpy(img.copy()).cuda()
    dgot = bb.min_filter(dimg, r)
    assert dgot.is_cuda
    np.testing.assert_array_equal(u32(dgot), u32(want))
    np.testing.assert_array_equal(u32(dimg), u32(img))          # the input is only read
    # in place, which the ABI allows: out == img
    assert bb.min_filter(dimg, r, out=dimg) is dimg
    np.testing.assert_array_equal(u32(dimg), u32(want))
    himg = img.copy()
    bb.min_filter(himg, r, out=himg)
    np.testing.assert_array_equal(u32(himg), u32(want))


def test_min_filter_nan_and_signed_zero(gpu, filter_refs):
    import torch
    img, want = filter_refs["special"]
    assert np.isnan(want).sum() == 7 * 7 * 5 and (np.signbit(want) & (want == 0)).any()   # (z 4 .. 8 of 9)
    np.testing.assert_array_equal(u32(bb.min_filter(img, 3)), u32(want))
    np.testing.assert_array_equal(u32(bb.min_filter(torch.from_numpy(img.copy()).cuda(), 3)), u32(want))


def test_min_filter_radius_beyond_the_kernels(gpu, lib):
    img = random_image((5, 200, 66), 3)
    out = np.zeros_like(img)
    st = lib.spim_min_filter(C.c_void_p(img.ctypes.data), (C.c_int64 * 3)(66, 200, 5), bb.MAX_RADIUS + 1, 0,
                             C.c_void_p(out.ctypes.data))
    assert st == -1 and "radius" in _lib.last_error() and not out.any()
    with pytest.raises(_lib.SpimDeconError):
        bb.min_filter(img, bb.MAX_RADIUS + 1)


def test_min_max(gpu, filter_refs):
    import torch
    for key, (img, _) in filter_refs.items():
        want = ar.min_max_fast(img)
        np.testing.assert_array_equal(u32(bb.min_max(img)), u32(want), err_msg=str(key))
        np.testing.assert_array_equal(u32(bb.min_max(torch.from_numpy(img.copy()).cuda())), u32(want))
    sp = filter_refs["special"][0]
    assert all(np.isnan(v) for v in bb.min_max(sp))                       # both are NaN
    z = sp.copy()
    z[np.isnan(z)] = 1.0
    z = np.where(z < 0, -z, z)                                            # (keeps -0) min is a zero: -0 wins
    mn, mx = bb.min_max(z)
    assert mn == 0 and np.signbit(mn)
    np.testing.assert_array_equal(u32((mn, mx)), u32(ar.min_max_fast(z)))
    mn, mx = bb.min_max(-z)                                               # max is a zero: +0 wins
    assert mx == 0 and not np.signbit(mx)
    inf = np.full((2, 3, 70), np.inf, np.float32)
    np.testing.assert_array_equal(u32(bb.min_max(inf)), u32((ar.FLOAT_MAX, np.inf)))


def test_threshold_bounds(gpu):
    import torch
    shape = (9, 31, 257)
    dims = [257, 31, 9]
    img = np.zeros(shape, np.float32)
    assert bb.threshold_bounds(img, 0.0) == (tuple(dims), (0, 0, 0), False)      # nothing above: the inverted box
    one = img.copy()
    one[0, 0, 0] = 1.0
    assert bb.threshold_bounds(one, 0.5) == ((0, 0, 0), (0, 0, 0), True)
    one = img.copy()
    one[8, 30, 256] = 1.0
    assert bb.threshold_bounds(one, 0.5) == ((256, 30, 8), (256, 30, 8), True)
    assert bb.threshold_bounds(torch.from_numpy(one).cuda(), 0.5) == ((256, 30, 8), (256, 30, 8), True)
    assert bb.threshold_bounds(one, 1.0) == (tuple(dims), (0, 0, 0), False)      # equal is not above
    v = np.float32(0.3)
    up = np.nextafter(v, np.float32(1))
    two = np.full(shape, v, np.float32)
    two[3, 17, 99] = up
    two[5, 4, 201] = up
    two[1, 1, 1] = np.nan
    between = (float(v) + float(up)) / 2                                         # between two adjacent floats
    assert float(v) < between < float(up)
    want = ar.threshold_bounds(two, between)
    assert want == ([99, 4, 3], [201, 17, 5], True)
    got = bb.threshold_bounds(two, between)
    assert (list(got[0]), list(got[1]), got[2]) == want
    rnd = random_image((70, 45, 130), 8)
    for thr in (0.9, 0.9999, 0.99999999, 1.0):
        got = bb.threshold_bounds(rnd, thr)
        assert (list(got[0]), list(got[1]), got[2]) == ar.threshold_bounds(rnd, thr)


@pytest.mark.parametrize("shape,r,background", [((9, 31, 257), 3, 5.0), ((70, 45, 130), 12, 40.0),
                                                ((3, 5, 7), 50, 5.0), ((3, 5, 67), 1, 5.0)])
def test_segment_bounds_is_the_composition(gpu, lib, shape, r, background):
    import torch
    img = np.abs(random_image(shape, 11)) * 0.02
    nz, ny, nx = shape
    img[nz // 8:nz - nz // 8, ny // 4:ny - ny // 8, nx // 3:nx - nx // 5] += 0.7      # survives r = 3 and 12
    dimg = torch.from_numpy(img).cuda()
    mn, mx = bb.min_max(dimg)
    thr = ar.threshold(mn, mx, background)
    filt = bb.min_filter(dimg, r)
    lo, hi, found = bb.threshold_bounds(filt, thr)
    plain = bb.segment_bounds(dimg, background, r)
    full = bb.segment_bounds(dimg, background, r, return_filtered=True)
    for res in (plain, full):
        np.testing.assert_array_equal(u32((res["min"], res["max"])), u32((mn, mx)))
        assert res["threshold"] == thr
        assert (res["bounds_min"], res["bounds_max"], res["found"]) == (lo, hi, found)
    assert "filtered" not in plain and full["filtered"].is_cuda
    np.testing.assert_array_equal(u32(full["filtered"]), u32(filt))
    assert found == (r < 50)
    # and the restatement, from a host image with the filtered image on the host
    want = ar.segment(img, background, r)
    host = bb.segment_bounds(img, background, r, return_filtered=True)
    assert (list(host["bounds_min"]), list(host["bounds_max"]), host["found"]) == (
        want["bounds_min"], want["bounds_max"], want["found"])
    assert host["threshold"] == want["threshold"]
    np.testing.assert_array_equal(u32(host["filtered"]), u32(want["filtered"]))
    np.testing.assert_array_equal(u32(filt), u32(want["filtered"]))
    # the C entry with every pairing of a host / device-resident image and `filtered`, and without it
    for src_dev in (False, True):
        for out_dev in (False, True, None):
            src, sp = staged(img, src_dev)
            out, op = staged(np.zeros_like(img), out_dev) if out_dev is not None else (None, None)
            res = _lib.SegmentResult()
            assert lib.spim_segment_bounds(sp, dims_of(img), background, r, 0, op, C.byref(res)) == 0
            np.testing.assert_array_equal(u32((res.min, res.max)), u32((mn, mx)))
            assert res.threshold == thr
            assert (tuple(res.bounds_min), tuple(res.bounds_max), bool(res.found)) == (lo, hi, found)
            if out is not None:
                np.testing.assert_array_equal(u32(out), u32(filt), err_msg=f"{src_dev} {out_dev}")


@pytest.fixture(scope="module")
def scene():
    views, models, params, truth = ar.scene()
    dims = [v.shape[::-1] for v in views]
    mb_min, _, _, fdims = ar.max_bounding_box(dims, models, params["downsampling"])
    return views, models, params, truth, mb_min, fdims


def test_auto_bounding_box_end_to_end(gpu, scene):
    import torch
    views, models, params, truth, mb_min, fdims = scene
    want = ar.auto_bounding_box(views, models, **params)          # over oracle/fusion_ref's fused image
    assert want["found"] and want["eff_radius"] >= 2
    for vs in (views, [torch.from_numpy(v).cuda() for v in views]):
        bb_min, bb_dims, det = bb.auto_bounding_box(vs, models, return_details=True, **params)
        assert det["found"]
        assert (list(bb_min), list(det["bb_max"]), list(bb_dims)) == (want["bb_min"], want["bb_max"], want["bb_dims"])
        assert (list(det["max_min"]), list(det["fused_dims"])) == (want["max_min"], want["fused_dims"])
        assert (det["radius_min"], det["eff_radius"]) == (want["radius_min"], want["eff_radius"])
        np.testing.assert_array_equal(u32((det["min"], det["max"])), u32((want["min"], want["max"])))
        assert det["threshold"] == want["threshold"]
        assert (list(det["bounds_min"]), list(det["bounds_max"])) == (want["bounds_min"], want["bounds_max"])
        assert bb.auto_bounding_box(vs, models, **params) == (bb_min, bb_dims)
    bb_max = det["bb_max"]
    for a in range(3):      # the ellipsoid is inside, the far bead is not
        assert bb_min[a] <= truth["ellipsoid_min"][a] and truth["ellipsoid_max"][a] <= bb_max[a]
    assert any(not (bb_min[a] <= truth["far_bead"][a] <= bb_max[a]) for a in range(3))
    # the fused image the library segmented is the one of the existing fusion entry
    from spim_registration_amd import input_prep
    fused = input_prep.fuse_weighted_average(views, models, mb_min, fdims, downsampling=float(params["downsampling"]),
                                             interpolation=0, use_blending=False)
    np.testing.assert_array_equal(u32(fused), u32(want["fused"]))


def test_auto_bounding_box_nothing_found(gpu):
    views = [np.zeros((12, 12, 12), np.float32)]
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    with pytest.raises(ValueError, match="no voxel"):
        bb.auto_bounding_box(views, [ident], downsampling=2)
    _, _, det = bb.auto_bounding_box(views, [ident], downsampling=2, return_details=True)
    assert not det["found"] and det["bounds_min"] == (6, 6, 6) and det["bounds_max"] == (0, 0, 0)
    bb.release_workspace(0)
    assert bb.min_max(views[0]) == (0, 0)          # (the workspace comes back)


def test_process_timepoint_auto_box(gpu):
    """bb_min="auto" is the same run as passing the estimated box explicitly"""
    import torch
    from spim_registration_amd import pipeline
    from spim_registration_amd import synthetic
    world = (48, 44, 40)         # the timepoint of tests/test_gpu_pipeline.py: rotations about y through the centre
    views, models = synthetic.make_timepoint_torch(world, world, 4, timepoint=1, config_id=41,
                                                   bead_density=1.0 / 9 ** 3, device="cuda:0")
    # plus a bright ball about the centre, which every view sees about its own centre; the beads stay
    # below 5 % of the range
    z, y, x = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device="cuda:0") for n in views[0].shape],
                             indexing="ij")
    ball = ((z - (world[2] - 1) / 2) ** 2 + (y - (world[1] - 1) / 2) ** 2 + (x - (world[0] - 1) / 2) ** 2) <= 81.0
    top = max(float(v.max()) for v in views)
    views = [torch.where(ball, torch.full_like(v, 40.0 * top), v).contiguous() for v in views]
    auto_bb = {"discarded_object_size": 6, "downsampling": 2}
    kw = dict(psf_size=(9, 9, 11), iterations=1)
    lines = []
    res = pipeline.process_timepoint(views, models, "auto", auto_bb=auto_bb, log=lines.append, **kw)
    bb_min, bb_dims = bb.auto_bounding_box(views, models, **auto_bb)
    assert res.bounding_box == (bb_min, bb_dims)
    assert any("automatic bounding box" in ln and str(bb_min) in ln for ln in lines)
    assert "auto_bounding_box" in res.ms
    assert tuple(res.psi.shape) == bb_dims[::-1]
    explicit = pipeline.process_timepoint(views, models, bb_min, bb_dims, **kw)
    assert explicit.bounding_box == (bb_min, bb_dims) and "auto_bounding_box" not in explicit.ms
    np.testing.assert_array_equal(u32(res.psi), u32(explicit.psi))
    with pytest.raises(ValueError, match="no voxel"):
        pipeline.process_timepoint([torch.zeros_like(v) for v in views], models, "auto", auto_bb=auto_bb, **kw)
    with pytest.raises(ValueError):
        pipeline.process_timepoint(views, models, "auto", bb_dims, **kw)
    with pytest.raises(ValueError):
        pipeline.process_timepoint(views, models, bb_min, bb_dims, auto_bb=auto_bb, **kw)
