"""CPU: the C ABI of the automatic bounding box -- argument errors, the host-only maximal box
against hand-computed corners and the restatement, and the compute entries failing loudly
without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import autobbox_ref as ar
from spim_registration_amd import _lib, boundingbox as bb

OK, ERR_ARG, ERR_DEVICE = 0, -1, -2
NO_GPU = pytest.mark.skipif(_lib.LIB_PATH.exists() and os.path.exists("/dev/kfd"), reason="GPU visible")
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def i3(*v):
    return (C.c_int64 * 3)(*v)


def max_box(lib, dims, models, ds):
    d = np.ascontiguousarray(np.asarray(dims, np.int64).reshape(-1, 3))
    m = np.ascontiguousarray(np.asarray(models, np.float64).reshape(-1, 12))
    out = [i3() for _ in range(4)]
    st = lib.spim_max_bounding_box(len(d), d.ctypes.data_as(_lib._pi64), m.ctypes.data_as(_lib._pd), ds, *out)
    return st, [list(o) for o in out]


def test_max_bounding_box_by_hand(lib):
    m = IDENT.copy()
    m[:, 3] = (-2.5, 0.5, 10.49)
    assert max_box(lib, [(10, 20, 30)], [m], 4) == (OK, [[-2, 1, 10], [7, 20, 39], [10, 20, 30], [2, 5, 7]])
    # a rotation by 90 degrees about z and a shift: x' = -y + 3, y' = x - 1.5
    r = np.array([[0, -1, 0, 3], [1, 0, 0, -1.5], [0, 0, 2, 0.25]], np.float64)
    # corners x 0..4, y 0..6, z 0..2 -> x' -3..3, y' -1.5..2.5 -> -1..3, z' 0.25..4.25 -> 0..4
    assert max_box(lib, [(5, 7, 3)], [r], 1) == (OK, [[-3, -1, 0], [3, 3, 4], [7, 5, 5], [7, 5, 5]])
    assert max_box(lib, [(10, 20, 30), (5, 7, 3)], [m, r], 3) == (
        OK, [[-3, -1, 0], [7, 20, 39], [11, 22, 40], [3, 7, 13]])
    assert bb.max_bounding_box([(10, 20, 30), (5, 7, 3)], [m, r], 3) == (
        (-3, -1, 0), (7, 20, 39), (11, 22, 40), (3, 7, 13))


def test_max_bounding_box_against_the_restatement(lib):
    rng = np.random.default_rng(4)
    for trial in range(20):
        nv = int(rng.integers(1, 4))
        dims = rng.integers(1, 60, size=(nv, 3))
        models = [np.hstack([np.eye(3) + rng.normal(0, 0.3, (3, 3)), rng.normal(0, 40, (3, 1))]) for _ in range(nv)]
        if trial % 4 == 0:     # land on .5 exactly
            models = [np.hstack([np.eye(3), np.round(rng.normal(0, 9, (3, 1))) + 0.5]) for _ in range(nv)]
        ds = int(rng.integers(1, 6))
        st, got = max_box(lib, dims, models, ds)
        assert st == OK and got == [list(v) for v in ar.max_bounding_box(dims, models, ds)]


def test_max_bounding_box_argument_errors(lib):
    bad = IDENT.copy()
    bad[1, 2] = np.nan
    inf = IDENT.copy()
    inf[0, 3] = np.inf
    for dims, models, ds in (([(10, 20, 30)], [bad], 1), ([(10, 20, 30)], [inf], 1), ([(10, 0, 30)], [IDENT], 1),
                             ([(10, 20, 30)], [IDENT], 0), ([(10, 20, 30)], [IDENT * 1e12], 1)):
        st, _ = max_box(lib, dims, models, ds)
        assert st == ERR_ARG and _lib.last_error(), (dims, ds)
    d = np.array([10, 20, 30], np.int64)
    m = IDENT.ravel().copy()
    assert lib.spim_max_bounding_box(1, None, m.ctypes.data_as(_lib._pd), 1, i3(), i3(), i3(), i3()) == ERR_ARG
    assert lib.spim_max_bounding_box(1, d.ctypes.data_as(_lib._pi64), None, 1, i3(), i3(), i3(), i3()) == ERR_ARG
    assert lib.spim_max_bounding_box(0, d.ctypes.data_as(_lib._pi64), m.ctypes.data_as(_lib._pd), 1, i3(), i3(), i3(),
                                     i3()) == ERR_ARG
    assert lib.spim_max_bounding_box(1, d.ctypes.data_as(_lib._pi64), m.ctypes.data_as(_lib._pd), 1, None, i3(), i3(),
                                     i3()) == ERR_ARG
    # fused_dims alone is optional
    assert lib.spim_max_bounding_box(1, d.ctypes.data_as(_lib._pi64), m.ctypes.data_as(_lib._pd), 1, i3(), i3(), i3(),
                                     None) == OK
    with pytest.raises(ValueError):
        bb.max_bounding_box([(10, 20, 30)], [bad])
    with pytest.raises(ValueError):
        bb.max_bounding_box([(10, 20, 30)], [IDENT, IDENT])


def test_defaults_and_layout(lib):
    p = _lib.AutoBBoxParams()
    p.device = 7
    lib.spim_autobbox_params_default(C.byref(p))
    assert (p.background, p.discarded_object_size, p.downsampling, p.device, p.src_on_device) == (5.0, 25, 4, 0, 0)
    assert list(p.reserved) == [0] * 8
    assert C.sizeof(_lib.SegmentResult) == 80 and C.sizeof(_lib.AutoBBoxParams) == 56
    assert C.sizeof(_lib.AutoBBoxResult) == 3 * 24 + 16 + 4 * 24 + 80
    assert bb.MAX_RADIUS == 64


def test_min_filter_tiles_needs_no_gpu(lib):
    import autobbox_cases as ac
    assert bb.min_filter_tiles() == (ac.LINES, ac.TILE_SMALL, ac.TILE_LARGE, ac.SMALL_RADIUS, ac.RED_BLOCK,
                                     ac.RED_GRID) == (64, 64, 128, 16, 256, 1024)
    lib.spim_min_filter_tiles(None)          # a null pointer is ignored


def test_image_argument_errors(lib):
    """Argument errors come before the device is looked at: these hold with and without a GPU."""
    img = np.ones((3, 4, 5), np.float32)
    out = np.zeros_like(img)
    ip, op, dims = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data), i3(5, 4, 3)
    mn, mx, found = C.c_float(), C.c_float(), C.c_int32()
    seg = _lib.SegmentResult()
    assert lib.spim_min_max(None, dims, 0, C.byref(mn), C.byref(mx)) == ERR_ARG
    assert lib.spim_min_max(ip, None, 0, C.byref(mn), C.byref(mx)) == ERR_ARG
    assert lib.spim_min_max(ip, dims, 0, None, C.byref(mx)) == ERR_ARG
    assert lib.spim_min_max(ip, i3(5, 0, 3), 0, C.byref(mn), C.byref(mx)) == ERR_ARG
    assert lib.spim_min_filter(None, dims, 1, 0, op) == ERR_ARG
    assert lib.spim_min_filter(ip, dims, 1, 0, None) == ERR_ARG
    assert lib.spim_min_filter(ip, i3(-1, 4, 3), 1, 0, op) == ERR_ARG
    for r in (0, -1, bb.MAX_RADIUS + 1, 1 << 20):
        assert lib.spim_min_filter(ip, dims, r, 0, op) == ERR_ARG and "radius" in _lib.last_error()
        assert lib.spim_segment_bounds(ip, dims, 5.0, r, 0, None, C.byref(seg)) == ERR_ARG
    assert lib.spim_threshold_bounds(None, dims, 0.5, 0, i3(), i3(), C.byref(found)) == ERR_ARG
    assert lib.spim_threshold_bounds(ip, dims, 0.5, 0, None, i3(), C.byref(found)) == ERR_ARG
    assert lib.spim_threshold_bounds(ip, dims, 0.5, 0, i3(), i3(), None) == ERR_ARG
    assert lib.spim_threshold_bounds(ip, i3(5, 4, 0), 0.5, 0, i3(), i3(), C.byref(found)) == ERR_ARG
    for bg in (0.0, 100.0, -1.0, 150.0, float("nan"), float("inf")):
        assert lib.spim_segment_bounds(ip, dims, bg, 1, 0, None, C.byref(seg)) == ERR_ARG
        assert "background" in _lib.last_error()
    assert lib.spim_segment_bounds(None, dims, 5.0, 1, 0, None, C.byref(seg)) == ERR_ARG
    assert lib.spim_segment_bounds(ip, dims, 5.0, 1, 0, None, None) == ERR_ARG
    assert lib.spim_segment_bounds(ip, i3(5, 4, 0), 5.0, 1, 0, None, C.byref(seg)) == ERR_ARG
    assert not out.any()


def auto_call(lib, views, models, **kw):
    vs = (_lib.ViewSource * len(views))()
    for i, (v, m) in enumerate(zip(views, models)):
        vs[i].img = _lib.fptr(v) if v is not None else None
        vs[i].dims[:] = [v.shape[2], v.shape[1], v.shape[0]] if v is not None else [4, 4, 4]
        vs[i].model[:] = [float(x) for x in np.asarray(m, np.float64).reshape(12)]
    p = _lib.AutoBBoxParams()
    lib.spim_autobbox_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    res = _lib.AutoBBoxResult()
    return lib.spim_auto_bounding_box(len(views), vs, C.byref(p), C.byref(res)), res


def test_auto_bounding_box_argument_errors(lib):
    v = np.ones((20, 20, 20), np.float32)
    bad = IDENT.copy()
    bad[2, 2] = -np.inf
    for kw in ({"background": 0.0}, {"background": 100.0}, {"background": float("nan")}, {"downsampling": 0},
               {"downsampling": -4}, {"discarded_object_size": -1},
               {"discarded_object_size": 2 * (bb.MAX_RADIUS + 1), "downsampling": 1},     # effR 65
               {"downsampling": 21}):                                                       # no fused voxel left
        st, _ = auto_call(lib, [v], [IDENT], **kw)
        assert st == ERR_ARG and _lib.last_error(), kw
    assert auto_call(lib, [v], [bad])[0] == ERR_ARG
    assert auto_call(lib, [None], [IDENT])[0] == ERR_ARG
    p, res = _lib.AutoBBoxParams(), _lib.AutoBBoxResult()
    lib.spim_autobbox_params_default(C.byref(p))
    vs = (_lib.ViewSource * 1)()
    assert lib.spim_auto_bounding_box(1, None, C.byref(p), C.byref(res)) == ERR_ARG
    assert lib.spim_auto_bounding_box(1, vs, None, C.byref(res)) == ERR_ARG
    assert lib.spim_auto_bounding_box(1, vs, C.byref(p), None) == ERR_ARG
    assert lib.spim_auto_bounding_box(0, vs, C.byref(p), C.byref(res)) == ERR_ARG
    assert lib.spim_bbox_release_workspace(-1) == ERR_ARG


@NO_GPU
def test_compute_entries_fail_loudly_without_gpu(lib):
    img = np.ones((3, 4, 5), np.float32)
    out = np.zeros_like(img)
    ip, op, dims = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data), i3(5, 4, 3)
    mn, mx, found = C.c_float(), C.c_float(), C.c_int32()
    seg = _lib.SegmentResult()
    for st in (lib.spim_min_max(ip, dims, 0, C.byref(mn), C.byref(mx)),
               lib.spim_min_filter(ip, dims, 1, 0, op),
               lib.spim_threshold_bounds(ip, dims, 0.5, 0, i3(), i3(), C.byref(found)),
               lib.spim_segment_bounds(ip, dims, 5.0, 1, 0, op, C.byref(seg)),
               auto_call(lib, [np.ones((20, 20, 20), np.float32)], [IDENT])[0]):
        assert st == ERR_DEVICE and "no HIP device" in _lib.last_error()
    assert not out.any()
    for call in (lambda: bb.min_max(img), lambda: bb.min_filter(img, 1), lambda: bb.threshold_bounds(img, 0.5),
                 lambda: bb.segment_bounds(img), lambda: bb.auto_bounding_box([np.ones((20, 20, 20), np.float32)],
                                                                                [IDENT])):
        with pytest.raises(_lib.SpimDeconError):
            call()
    # releasing a workspace nobody made is not an error
    assert lib.spim_bbox_release_workspace(0) == OK
