"""CPU: the Difference-of-Mean restatement (tests/dom_ref.py) against itself (literal
loops vs vectorised), against direct box sums and the committed golden file; the host-only
part of the C ABI (defaults, diameters, every bad argument) through the built library."""
import ctypes as C
import os

import numpy as np
import pytest

import dom_ref as dr
from spim_registration_amd import _lib, dom, pipeline

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dom.npz")
NAN = float("nan")
OK, ERR_ARG = 0, -1     # SPIMDECON_OK, SPIMDECON_ERR_ARG


def _volume(shape, seed, scale=900.0):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) - 0.2) * scale).astype(np.float32)   # negative and fractional values too


@pytest.mark.parametrize("shape,s1,s2", [
    ((9, 10, 11), (3, 3, 3), (5, 5, 5)),
    ((12, 11, 13), (5, 5, 5), (7, 7, 7)),
    ((16, 9, 10), (5, 5, 9), (7, 7, 13)),       # anisotropic: sigma z = 0.25
    ((10, 11, 12), (7, 7, 7), (5, 5, 5)),       # radius1 > radius2
])
def test_literal_equals_vectorised(shape, s1, s2):
    img = _volume(shape, 3)
    mn, mx = dr.min_max(img)
    a = dr.dom_image(img, s1, s2, mn, mx)
    b = dr.dom_image_literal(img, s1, s2, mn, mx)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    hm = [max(s1[i], s2[i]) // 2 for i in range(3)]
    inner = a[hm[2]:shape[0] - hm[2], hm[1]:shape[1] - hm[1], hm[0]:shape[2] - hm[0]]
    assert inner.size > 0 and np.all(inner != 0)
    frame = a.copy()
    frame[hm[2]:shape[0] - hm[2], hm[1]:shape[1] - hm[1], hm[0]:shape[2] - hm[0]] = 0
    assert not frame.any()
    np.testing.assert_array_equal(dr.integral_image(img), dr.integral_image_literal(img))


def test_direct_box_sums_equal_integral_sums_with_saturating_values():
    """Rule 3: any order of summation gives the reference's s1 / s2, also past 2^63."""
    img = _volume((9, 10, 11), 5)
    rng = np.random.default_rng(6)
    img[rng.random(img.shape) < 0.3] = 3e9     # -> 2^31 - 1
    img[rng.random(img.shape) < 0.3] = -3e9    # -> -2^31
    img[0, 0, 0] = NAN
    img[1, 2, 3] = np.inf
    integral = dr.integral_image(img)
    for s, hm in (((3, 3, 3), (2, 2, 2)), ((5, 5, 5), (2, 2, 2)), ((5, 3, 7), (2, 2, 3))):
        got = dr.box_sums(integral, s, hm)
        want = dr.direct_box_sums(img, s, hm)
        assert np.abs(want).max() > 2 ** 31
        np.testing.assert_array_equal(got, want)


def test_integral_sums_wrap_like_a_long():
    """Sums past 2^63 wrap in the integral image and in its corner differences alike."""
    img = np.full((4, 5, 6), 3e9, np.float32)
    integral = dr.integral_image(img).astype(object) * 2 ** 33     # exact Python ints, scaled past 2^63
    wrapped = np.vectorize(dr._wrap, otypes=[np.int64])(integral)
    got = dr.box_sums(wrapped, (3, 3, 3), (1, 1, 1))
    assert np.all(got == dr._wrap(27 * (2 ** 31 - 1) * 2 ** 33))


@pytest.mark.parametrize("r1,r2,sigma,s1,s2", [
    (2, 3, (0.5, 0.5, 0.5), (5, 5, 5), (7, 7, 7)),
    (1, 2, (0.5, 0.5, 0.5), (3, 3, 3), (5, 5, 5)),
    (2, 3, (0.5, 0.5, 0.25), (5, 5, 9), (7, 7, 13)),
    (1, 1, (0.5, 0.5, 0.5), (3, 3, 3), (5, 5, 5)),       # the minima 3 and 5
    (3, 5, (1.0, 0.6, 0.5), (5, 7, 7), (7, 9, 11)),       # 1.5 -> 2 and 2.5 -> 3: .5 rounds up
    (15, 16, (0.5, 0.5, 0.5), (31, 31, 31), (33, 33, 33)),
])
def test_diameter_rule(lib, r1, r2, sigma, s1, s2):
    assert dr.box_diameters(r1, r2, sigma) == (s1, s2)
    assert dom.box_diameters(r1, r2, sigma) == (s1, s2)


def test_cast_table():
    f = np.float32([1.9, -1.9, NAN, 3e9, -3e9, np.inf, -np.inf, 0.999, -0.0, 2147483520.0])
    want = [1, -1, 0, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 0, 0, 2147483520]
    got = dr.java_int(f)
    assert got.dtype == np.int64 and got.tolist() == want


def test_min_max_rule():
    img = np.float32([[[1.0, 5.0, -2.0]]])
    assert dr.min_max(img) == (-2.0, 5.0)
    assert dr.min_max(img, 0.0, 10.0) == (0.0, 10.0)
    assert dr.min_max(img, 3.0, 3.0) == (-2.0, 5.0)          # equal: the image's own
    assert dr.min_max(img, np.inf, 3.0) == (-2.0, 5.0)
    assert all(np.isnan(v) for v in dr.min_max(np.float32([[[1.0, NAN]]])))   # Math.min keeps a NaN


def test_params_default(lib):
    p = _lib.DomParams()
    lib.spim_dom_params_default(C.byref(p))
    assert (p.radius1, p.radius2, p.localization, p.find_min, p.find_max, p.ij_threads, p.device) == \
        (2, 3, 0, 0, 1, 8, 0)
    assert p.threshold == np.float32(0.02) and list(p.image_sigma) == [0.5, 0.5, 0.5]
    assert np.isnan(p.min_intensity) and np.isnan(p.max_intensity)
    s1, s2 = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    assert lib.spim_dom_diameters(C.byref(p), s1, s2) == OK
    assert list(s1) == [5, 5, 5] and list(s2) == [7, 7, 7]


def _call(lib, fn, p, img=True, dims=(8, 8, 8), count=True, out=True):
    """status of spim_dom_compute / spim_dom_interest_points on a host volume"""
    a = np.zeros(dims[::-1] if all(d > 0 for d in dims) else (1, 1, 1), np.float32)
    d = (C.c_int64 * 3)(*dims)
    n = C.c_int64(-1)
    if fn == "compute":
        buf = (_lib.Peak * 4)()
        return lib.spim_dom_compute(_lib.fptr(a) if img else None, d, C.byref(p) if p is not None else None, None,
                                    buf if out else None, 4, C.byref(n) if count else None)
    buf = (_lib.InterestPointC * 4)()
    return lib.spim_dom_interest_points(_lib.fptr(a) if img else None, d, C.byref(p) if p is not None else None,
                                        None, buf if out else None, 4, C.byref(n) if count else None)


BAD = [
    ("radius1", 0), ("radius2", 0), ("radius1", -3), ("ij_threads", 0), ("localization", 2), ("localization", -1),
    ("image_sigma", (0.5, 0.0, 0.5)), ("image_sigma", (-1.0, 0.5, 0.5)), ("image_sigma", (0.5, 0.5, NAN)),
    ("image_sigma", (np.inf, 0.5, 0.5)),
]


@pytest.mark.parametrize("fn", ["compute", "points"])
@pytest.mark.parametrize("field,value", BAD)
def test_bad_parameters_are_refused_without_a_gpu(lib, fn, field, value):
    p = _lib.DomParams()
    lib.spim_dom_params_default(C.byref(p))
    if field == "image_sigma":
        for i in range(3):
            p.image_sigma[i] = value[i]
    else:
        setattr(p, field, value)
    assert _call(lib, fn, p) == ERR_ARG
    if field != "localization" and field != "ij_threads":
        s1, s2 = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        assert lib.spim_dom_diameters(C.byref(p), s1, s2) == ERR_ARG


@pytest.mark.parametrize("fn", ["compute", "points"])
def test_bad_arguments_are_refused_without_a_gpu(lib, fn):
    p = _lib.DomParams()
    lib.spim_dom_params_default(C.byref(p))
    assert _call(lib, fn, None) == ERR_ARG
    assert _call(lib, fn, p, img=False) == ERR_ARG
    assert _call(lib, fn, p, count=False) == ERR_ARG
    for dims in ((0, 8, 8), (8, -1, 8), (8, 8, 0)):
        assert _call(lib, fn, p, dims=dims) == ERR_ARG
    d = (C.c_int64 * 3)(8, 8, 8)
    n = C.c_int64(0)
    a = np.zeros((8, 8, 8), np.float32)
    if fn == "compute":
        assert lib.spim_dom_compute(_lib.fptr(a), None, C.byref(p), None, None, 0, C.byref(n)) == ERR_ARG
    else:
        assert lib.spim_dom_interest_points(_lib.fptr(a), None, C.byref(p), None, None, 0, C.byref(n)) == ERR_ARG
    s1 = (C.c_int32 * 3)()
    assert lib.spim_dom_diameters(None, s1, s1) == ERR_ARG
    assert lib.spim_dom_diameters(C.byref(p), None, s1) == ERR_ARG


def test_localization_2_message(lib):
    p = _lib.DomParams()
    lib.spim_dom_params_default(C.byref(p))
    p.localization = 2
    assert _call(lib, "points", p) == ERR_ARG
    assert b"localization must be 0 (none) or 1 (quadratic)" in lib.spimdecon_last_error()


def test_pipeline_rejects_an_unknown_detector():
    with pytest.raises(ValueError, match="detector"):
        pipeline.process_timepoint([], [], (0, 0, 0), (8, 8, 8), detector="log")
    with pytest.raises(ValueError, match="detector"):
        pipeline.Pipeline(detector=None).process([], [], (0, 0, 0), (8, 8, 8))


def test_golden_equals_the_restatement():
    g = np.load(GOLDEN)
    img = g["img"]
    assert img.shape == (24, 28, 32) and img.dtype == np.float32
    pts, peaks, d = dr.process_dom(img, find_min=True, find_max=True)
    np.testing.assert_array_equal(d.view(np.uint32), g["dom"].view(np.uint32))
    assert len(peaks) == len(g["peaks"]) > 5
    assert [(p[0], p[1], p[2], int(p[4]), int(p[5])) for p in peaks] == [tuple(r) for r in g["peaks"].tolist()]
    np.testing.assert_array_equal(np.float32([p[3] for p in peaks]), g["intensity"])
    assert g["peaks"][:, 4].sum() > 0 and g["peaks"][:, 3].sum() > 0     # maxima and minima


@pytest.mark.parametrize("name", list(dr.Z_CHUNK_CASES))
def test_z_chunk_cases_start_a_second_chunk(name):
    """The shapes of tests/test_gpu_dom.py::test_dom_across_z_chunks, from dom_tile's rule
    restated (dom_ref.z_chunks): two chunks each, ragged or full as the name says."""
    shape, kw, chunks = dr.Z_CHUNK_CASES[name]
    s1, s2 = dr.box_diameters(kw.get("radius1", 2), kw.get("radius2", 3), kw.get("image_sigma", (0.5, 0.5, 0.5)))
    hm = [max(a, b) // 2 for a, b in zip(s1, s2)]
    assert dr.z_chunks(shape[0], hm[2]) == chunks and len(chunks) == 2
    assert all(n > 2 * h for n, h in zip(shape[::-1], hm)) and np.prod(shape) < 250_000
    if name == "anisotropic":
        assert hm[2] != hm[0] and 8 * hm[2] > 64
    if name == "largest_box":
        assert dr.tile_columns(hm) > 8 * 256 >= dr.tile_columns([3, 3, 3])      # 16 columns per thread


def test_sparse_integers_tie_across_the_chunk_seam():
    img = dr.sparse_integer_volume()
    pts, peaks, d = dr.process_dom(img, threshold=0.0, find_min=True, find_max=True)
    assert dr.z_chunks(img.shape[0], 3) == [64, 5]
    seam = 3 + 64                                   # the first output plane of the second chunk
    inner = d[3:-3, 3:-3, 3:-3]
    assert np.unique(inner).size < inner.size // 20      # ties
    # plateau voxels (every neighbour equal) are candidates, on both sides of the seam
    flat = {p[:3] for p in peaks if np.all(d[p[2] - 1:p[2] + 2, p[1] - 1:p[1] + 2, p[0] - 1:p[0] + 2] == d[p[2], p[1], p[0]])}
    assert {z for _, _, z in flat} >= {seam - 1, seam} and all(p[5] for p in peaks if p[:3] in flat)
