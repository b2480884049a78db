"""CPU: the restatement of the reference's downsampling (tests/downsample_ref.py) against
known answers, and the host-only parts of the library and of
``spim_registration_amd.downsample`` against the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import downsample_ref as dr
from oracle import dog_ref
from spim_registration_amd import _lib, downsample as ds

OK, ERR_ARG = 0, -1


def f32(*v):
    return np.array(v, np.float64).astype(np.float32)


def test_known_answers():
    np.testing.assert_array_equal(dr.simple2x(f32(1, 2, 3, 4), 0), f32(4 / 3, 8 / 3))
    np.testing.assert_array_equal(dr.simple2x(f32(0, 1, 2, 3, 4, 5, 6), 0), f32(1 / 3, 2.0, 11 / 3))
    # by hand: (1 + 2 * 0.5) / 1.5, (3 + 2 * 0.5) / 1.5; (0 + 0.5) / 1.5, (0.5 + 2 + 1.5) / 2, (4 + 1.5) / 1.5
    np.testing.assert_array_equal(dr.simple2x_literal([1, 2, 3, 4]), f32(2 / 1.5, 4 / 1.5))
    np.testing.assert_array_equal(dr.simple2x_literal([0, 1, 2, 3, 4, 5, 6]), f32(0.5 / 1.5, 2.0, 5.5 / 1.5))


def test_last_element_of_an_odd_line_is_unread():
    a = dr.simple2x(f32(1, 2, 3, 4), 0)
    np.testing.assert_array_equal(dr.simple2x(f32(1, 2, 3, 4, 5), 0), a)
    np.testing.assert_array_equal(dr.simple2x(f32(1, 2, 3, 4, np.nan), 0), a)
    # and of an even line: in[2m - 1]
    np.testing.assert_array_equal(dr.simple2x(f32(1, 2, 3, np.nan), 0), a)


def test_vectorised_restatement_is_the_literal_loop():
    rng = np.random.default_rng(3)
    for n in range(4, 40):
        line = ((rng.random(n) - 0.3) * 1000).astype(np.float32)
        np.testing.assert_array_equal(dr.simple2x(line, 0), dr.simple2x_literal(line))
    vol = rng.random((5, 6, 9)).astype(np.float32)
    for axis in range(3):
        got = dr.simple2x(vol, axis)
        for idx in np.ndindex(*[s for a, s in enumerate(vol.shape) if a != axis]):
            sl = list(idx)
            sl.insert(axis, slice(None))
            np.testing.assert_array_equal(got[tuple(sl)], dr.simple2x_literal(vol[tuple(sl)]))


def test_chain_order_is_x_then_y_then_z():
    """Each level rounds to float: the reference's order (all x, all y, all z) is not the
    per-level interleaving bit for bit."""
    rng = np.random.default_rng(5)
    vol = (rng.random((9, 21, 22)) * 4000).astype(np.float32)
    want = vol
    for axis in (2, 2, 1, 1, 0):
        want = dr.simple2x(want, axis)
    np.testing.assert_array_equal(dr.downsample(vol, 4, 2), want)
    other = vol
    for axis in (2, 1, 2, 1, 0):
        other = dr.simple2x(other, axis)
    assert want.shape == other.shape == (4, 5, 5) and np.any(want != other)


def dims_call(lib, dims, factor):
    od = (C.c_int64 * 3)()
    st = lib.spim_downsample_dims((C.c_int64 * 3)(*dims), (C.c_int32 * 3)(*factor), od)
    return st, tuple(od)


def test_dims_through_the_library(lib):
    """spim_downsample_dims is host only: it works without a GPU."""
    assert dims_call(lib, (23, 16, 9), (8, 8, 1)) == (OK, (2, 2, 9))       # 23 -> 11 -> 5 -> 2, 16 -> 8 -> 4 -> 2
    assert dims_call(lib, (23, 16, 9), (4, 2, 2)) == (OK, (5, 8, 4))
    assert dims_call(lib, (3, 2, 1), (1, 1, 1)) == (OK, (3, 2, 1))
    assert ds.out_dims((9, 16, 23), 8, 1) == dr.out_dims((9, 16, 23), 8, 1) == (9, 2, 2)
    for dims, factor in (((15, 16, 16), (8, 1, 1)),      # 15 -> 7 -> 3: the third level's input is 3 long
                         ((16, 15, 16), (1, 8, 1)), ((16, 16, 15), (1, 1, 8)),
                         ((3, 16, 16), (2, 1, 1)), ((16, 3, 16), (1, 2, 1)), ((16, 16, 3), (1, 1, 2)),
                         ((16, 16, 16), (3, 1, 1)), ((16, 16, 16), (1, 16, 1)), ((16, 16, 16), (1, 1, 0)),
                         ((0, 16, 16), (1, 1, 1))):
        st, _ = dims_call(lib, dims, factor)
        assert st == ERR_ARG and _lib.last_error(), (dims, factor)
    assert lib.spim_downsample_dims(None, (C.c_int32 * 3)(1, 1, 1), (C.c_int64 * 3)()) == ERR_ARG
    with pytest.raises(ValueError):
        ds.out_dims((16, 16, 15), 8, 1)
    with pytest.raises(ValueError):
        ds.out_dims((16, 16, 16), 3, 1)
    for n in range(4, 70):
        for f in (1, 2, 4, 8):
            try:
                want = dr.out_dims((n, 5, 5), 1, f)
            except ValueError:
                want = None
            st, od = dims_call(lib, (5, 5, n), (1, 1, f))
            assert (od[::-1] if st == OK else None) == want


FACTOR_TABLE = [   # voxel, ds_z, "less", "more" (None: beyond 8x, an error)
    ((0.5, 0.5, 2.0), 1, 4, 4),
    ((0.4, 0.4, 2.0), 1, 4, 8),
    ((1.0, 1.0, 1.0), 1, 1, 1),
    ((1.0, 1.0, 0.25), 1, 1, 1),          # the reference's 0, clamped
    ((0.1, 0.1, 2.0), 1, None, None),
    ((0.5, 0.7, 1.0), 2, 4, 4),           # min(x, y); the z factor counts
    ((0.73, 0.73, 2.0), 1, 2, 4),
]


@pytest.mark.parametrize("voxel,ds_z,less,more", FACTOR_TABLE)
def test_factor_rule(lib, voxel, ds_z, less, more):
    for choice, is_more, want in (("match_z_less", False, less), ("match_z_more", True, more)):
        raw = dr.downsample_factor(is_more, ds_z, voxel)
        if want is None:
            assert raw > 8
            with pytest.raises(ValueError, match="above 8"):
                ds.downsample_factor(choice, ds_z, voxel)
        else:
            assert max(raw, 1) == want
            assert ds.downsample_factor(choice, ds_z, voxel) == want
    assert dr.downsample_factor(False, 1, (1.0, 1.0, 0.25)) == 0      # what the reference would scale by


def test_factor_rule_arguments(lib):
    assert [ds.downsample_factor(f) for f in (1, 2, 4, 8)] == [1, 2, 4, 8]
    for bad in (0, 3, 16, 2.5, "match_z", "less"):
        with pytest.raises(ValueError):
            ds.downsample_factor(bad, 1, (1, 1, 1))
    with pytest.raises(ValueError, match="voxel_size"):
        ds.downsample_factor("match_z_less")
    f = C.c_int32(0)
    for voxel, dz in (((0.0, 1.0, 1.0), 1), ((1.0, 1.0, float("nan")), 1), ((1.0, -1.0, 1.0), 1),
                      ((1.0, 1.0, 1.0), 3)):
        assert lib.spim_downsample_factor_xy(0, dz, (C.c_double * 3)(*voxel), C.byref(f)) == ERR_ARG
    assert lib.spim_downsample_factor_xy(0, 1, None, C.byref(f)) == ERR_ARG


def test_correct_for_downsampling():
    rng = np.random.default_rng(9)
    pts = (rng.random((17, 3)) - 0.2) * 300
    pts[3] = (-0.0, 0.0, 5.5)
    for xy, z in ((1, 1), (2, 1), (4, 2), (8, 8), (1, 4)):
        got = ds.correct_for_downsampling(pts, xy, z)
        want = dr.correct_for_downsampling(pts, xy, z)
        assert got.dtype == np.float64 and got.shape == (17, 3)
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
        np.testing.assert_array_equal(got, pts * [xy, xy, z])
    assert ds.correct_for_downsampling(np.zeros((0, 3)), 2, 2).shape == (0, 3)


@pytest.mark.parametrize("kind", ["brightest", "median", "weakest"])
def test_limit_detections(kind):
    rng = np.random.default_rng(11)
    # ties in |intensity| (also between a negative and a positive value), negative intensities
    inten = rng.choice(np.float32([0.5, -0.5, 0.25, -1.0, 1.0, 0.125, 2.0, -3.0]), size=23).astype(np.float32)
    pts = rng.random((23, 3)) * 100
    assert len(set(np.abs(inten).tolist())) < 23
    for n in (23, 22, 9, 4):
        for limit in (0, 1, 2, 3, 4, 5, 8, 21, 22, 23, 24, 100):
            p, i = ds.limit_detections(pts[:n], inten[:n], limit, kind)
            sel = dr.limit_list(pts[:n], inten[:n], limit, ds.LIMIT_KINDS[kind])
            np.testing.assert_array_equal(p, pts[:n][sel])
            np.testing.assert_array_equal(i, inten[:n][sel])
            if n <= limit:      # returned unchanged, in the given order
                assert sel == list(range(n))
            elif kind == "median":
                assert len(sel) == limit // 2 * 2 + 1
            else:
                assert len(sel) == limit
    with pytest.raises(ValueError):
        ds.limit_detections(pts, inten, 3, "max")


def test_limit_detections_order():
    inten = np.float32([0.1, -0.9, 0.5, 0.9, -0.3, 0.7])
    pts = np.arange(18.0).reshape(6, 3)
    # stable: -0.9 (index 1) stays before 0.9 (index 3)
    assert ds.limit_detections(pts, inten, 3, "brightest")[1].tolist() == np.float32([-0.9, 0.9, 0.7]).tolist()
    assert ds.limit_detections(pts, inten, 2, "weakest")[1].tolist() == np.float32([0.1, -0.3]).tolist()
    # sorted: -0.9 0.9 0.7 0.5 -0.3 0.1; median 3, range 2 .. 4 from the end: indices 3, 2, 1
    assert ds.limit_detections(pts, inten, 2, "median")[1].tolist() == np.float32([0.5, 0.7, 0.9]).tolist()


def blob_volume(centre_zyx, shape, sigma=4.0):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    d2 = (z - centre_zyx[0]) ** 2 + (y - centre_zyx[1]) ** 2 + (x - centre_zyx[2]) ** 2
    return np.exp(-d2 / (2 * sigma * sigma)).astype(np.float32)


BLOB_SHAPE, BLOB_CENTRE = (58, 60, 68), (2 * 14, 4 * 7, 4 * 9)      # (z, y, x); >= 24 voxels from every face


def test_centred_blob_restated():
    """Output voxel p is centred on input voxel factor * p: a blob centred on (4a, 4b, 2c)
    is detected there after the pure scale, with no half-voxel offset (zero by symmetry:
    only rounding remains)."""
    assert all(min(c, n - 1 - c) >= 24 for c, n in zip(BLOB_CENTRE, BLOB_SHAPE))
    small = dr.downsample(blob_volume(BLOB_CENTRE, BLOB_SHAPE), 4, 2)
    pts, _ = dog_ref.process_dog(small, localization=1)
    assert len(pts) == 1
    pos = dr.correct_for_downsampling([pts[0][:3]], 4, 2)[0]
    assert np.abs(pos - BLOB_CENTRE[::-1]).max() < 1e-3, pos


@pytest.mark.skipif(_lib.LIB_PATH.exists() and os.path.exists("/dev/kfd"), reason="GPU visible")
def test_downsample_fails_loudly_without_gpu(lib):
    img = np.ones((4, 4, 4), np.float32)
    out = np.zeros((4, 2, 2), np.float32)
    st = lib.spim_downsample(img.ctypes.data, (C.c_int64 * 3)(4, 4, 4), (C.c_int32 * 3)(2, 2, 1), 0,
                             out.ctypes.data)
    assert st == -2 and "no HIP device" in _lib.last_error()
    assert not out.any()
    with pytest.raises(_lib.SpimDeconError):
        ds.downsample(img, 2, 1)
    # argument errors come first, as for every entry point
    st = lib.spim_downsample(img.ctypes.data, (C.c_int64 * 3)(3, 4, 4), (C.c_int32 * 3)(2, 2, 1), 0,
                             out.ctypes.data)
    assert st == ERR_ARG
