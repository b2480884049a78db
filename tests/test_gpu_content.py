"""GPU: content-based fusion weights (ContentBased.approximateEntropy) and the weighted-
average fusion that uses them, against the restatement in tests/content_ref.py."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import content_ref as cr
from conftest import rel_l2
from oracle import fusion_ref as fr
from oracle import input_ref as ir
from spim_registration_amd import _lib
from spim_registration_amd.input_prep import content_based_weights, fuse_weighted_average

pytestmark = pytest.mark.gpu

ERR_ARG = -1

# name: (shape [z, y, x], sigma1 (x, y, z), sigma2 (x, y, z))
CASES = {
    "a_multifold_z": ((20, 45, 70), (3, 3, 2), (6, 6, 8)),          # z radius 24 > 19
    "b_long_kernels": ((50, 24, 300), (20, 5, 20), (40, 8, 40)),     # 121 / 241 taps, radius 120 on 50 planes
    "c_one_plane": ((1, 33, 50), (4, 4, 4), (7, 7, 7)),
    "d_tile_edges": ((9, 31, 257), (1.5, 1.5, 1.5), (3, 3, 3)),
    "s_staging": ((3, 5, 67), (1.5, 1.5, 1.5), (3, 3, 3)),           # no extent a multiple of any tile
}


def image(shape, seed):
    """Beads and a smooth gradient over noise: content that the weights respond to."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    img = 5 + 10 * rng.random(shape) + 20 * x / max(nx - 1, 1) + 8 * y / max(ny - 1, 1)
    for _ in range(6):
        cz, cy, cx = rng.integers(0, nz), rng.integers(0, ny), rng.integers(0, nx)
        img += 60 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / 8.0)
    return img.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    shape, s1, s2 = CASES[name]
    img = image(shape, seed=len(name))
    w64 = cr.content_weights(img, s1, s2, "f64")
    w32 = cr.content_weights(img, s1, s2, "f32")
    for a in (img, w64, w32):
        a.setflags(write=False)
    return img, s1, s2, w64, w32


def check_against_restatement(name, got, w64, w32):
    """GPU error against the f64 restatement <= 8 x the error of the restatement's own
    f32 run (the stand-in for the reference's float FFT)."""
    d32 = float(np.abs(w32.astype(np.float64) - w64).max())
    dgpu = float(np.abs(got.astype(np.float64) - w64).max())
    print(f"content weights {name}: d32 {d32:.3e}  gpu {dgpu:.3e}  ratio {dgpu / d32 if d32 else math.inf:.2f}")
    assert dgpu <= 8 * d32, (name, dgpu, d32)


@pytest.mark.parametrize("name", list(CASES))
def test_weights_match_restatement(gpu, name):
    img, s1, s2, w64, w32 = case(name)
    got = content_based_weights(img, s1, s2)
    assert got.shape == img.shape and got.dtype == np.float32
    assert got.min() == 0.0 and got.max() == 1.0 and w64.min() == 0.0 and w64.max() == 1.0
    check_against_restatement(name, got, w64, w32)


def test_constant_image_skips_normalisation(gpu):
    """Case e: max - min == 0, normalizeImage leaves the blurred squares as they are."""
    img = np.full((7, 20, 70), 7.25, np.float32)
    s1, s2 = (3, 2, 1.5), (5, 4, 3)
    w64 = cr.content_weights(img, s1, s2, "f64")
    w32 = cr.content_weights(img, s1, s2, "f32")
    assert w64.min() == w64.max()                       # the restatement took the skip branch
    got = content_based_weights(img, s1, s2)
    check_against_restatement("e_constant", got, w64, w32)
    # every voxel sums the same values in the same order: exactly uniform, so skipped; what
    # is left is the square of the blur's rounding on 7.25 (a few ulp of 4.8e-7), not [0, 1]
    assert got.min() == got.max()
    assert 0.0 <= float(got.max()) < 1e-9


def rot_z(deg, zscale=1.3):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.diag([1.0, 1.0, zscale])


@functools.lru_cache(maxsize=None)
def fusion_inputs():
    shape, s1, s2 = CASES["a_multifold_z"]
    srcs = [image(shape, 11), image(shape, 12)]
    models = []
    for deg, tr in ((0.0, (0.0, 0.0, 0.0)), (7.0, (9.0, 1.5, 2.25))):
        m = np.zeros((3, 4))
        m[:, :3] = rot_z(deg)
        m[:, 3] = tr
        models.append(m)
    bb_min, bb_dims = (-6, -4, -2), (84, 56, 30)
    borders, ranges = [(0, 0, 0), (1, 1, 0)], [(10, 8, 4), (8, 10, 5)]
    w64 = [cr.content_weights(s, s1, s2, "f64") for s in srcs]
    covered = np.zeros((bb_dims[2], bb_dims[1], bb_dims[0]), bool)
    for s, m in zip(srcs, models):
        t = ir.image_positions(m, bb_min, bb_dims)
        covered |= ((t >= 0).all(-1) & (t[..., 0] < s.shape[2]) & (t[..., 1] < s.shape[1])
                    & (t[..., 2] < s.shape[0]))
    return srcs, models, bb_min, bb_dims, borders, ranges, s1, s2, w64, covered


@pytest.mark.parametrize("blend", [True, False])
def test_fusion_elementwise_with_gpu_weights(gpu, blend):
    """The GPU's own weight images through the restatement's fuse: isolates the zero-
    extended sampling and the weight product from the Gaussian's rounding."""
    srcs, models, bb_min, bb_dims, borders, ranges, s1, s2, _, covered = fusion_inputs()
    ws = [content_based_weights(s, s1, s2) for s in srcs]
    got = fuse_weighted_average(srcs, models, bb_min, bb_dims, 1.0, 1, blend, borders, ranges,
                                use_content_based=True, content_sigma1=s1, content_sigma2=s2)
    want = cr.fuse(srcs, models, ws, bb_min, bb_dims, 1.0, 1, blend, borders, ranges)
    assert covered.mean() > 0.5 and not covered.all()
    assert (got[~covered] == 0).all() and (want > 0).mean() > 0.4
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-4)
    # and the weights matter: the result is neither the blended nor the plain fusion
    plain = fr.fuse_weighted_average(srcs, models, bb_min, bb_dims, 1.0, 1, blend, borders, ranges)
    assert np.abs(got - plain).max() > 1e-2


@pytest.mark.parametrize("blend", [True, False])
def test_fusion_end_to_end(gpu, blend):
    """Against the restatement run with its own f64 weights: rel-L2 <= 1e-4 (where the
    weight sum is tiny an elementwise bound would not be fair to either side)."""
    srcs, models, bb_min, bb_dims, borders, ranges, s1, s2, w64, _ = fusion_inputs()
    got = fuse_weighted_average(srcs, models, bb_min, bb_dims, 1.0, 1, blend, borders, ranges,
                                use_content_based=True, content_sigma1=s1, content_sigma2=s2)
    want = cr.fuse(srcs, models, w64, bb_min, bb_dims, 1.0, 1, blend, borders, ranges)
    err = rel_l2(got, want)
    print(f"content fusion end to end (blending {blend}): rel-L2 {err:.3e}")
    assert err <= 1e-4


def test_per_view_sigmas(gpu):
    """sigma1 / sigma2 as one triple per view reach the matching view."""
    srcs, models, bb_min, bb_dims, _, _, s1, s2, _, _ = fusion_inputs()
    p1, p2 = [s1, (2, 2, 2)], [s2, (4, 3, 5)]
    ws = [content_based_weights(s, a, b) for s, a, b in zip(srcs, p1, p2)]
    got = fuse_weighted_average(srcs, models, bb_min, bb_dims, use_blending=False, use_content_based=True,
                                content_sigma1=p1, content_sigma2=p2)
    want = cr.fuse(srcs, models, ws, bb_min, bb_dims)
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-4)


def test_weights_inside_fusion_are_the_stand_alone_weights(gpu):
    """Identity models, integer positions: the n-linear sample of a weight image is the
    weight itself.  One view: (v * w) / w in double returns I exactly where w > 0, and 0
    where w == 0.  Two views on the same grid: (v0 * w0 + v1 * w1) / (w0 + w1) evaluated
    in double from the stand-alone weights must equal the fusion call's output bit for
    bit, which holds only if the call computed the same weight bits."""
    img, s1, s2, _, _ = case("d_tile_edges")
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    dims = (img.shape[2], img.shape[1], img.shape[0])
    w = content_based_weights(img, s1, s2)
    got = fuse_weighted_average([img], [ident], (0, 0, 0), dims, use_blending=False, use_content_based=True,
                                content_sigma1=s1, content_sigma2=s2)
    assert (w == 0).sum() >= 1
    # v * w / w in double, rounded to float, is v exactly for float v and w
    np.testing.assert_array_equal(got, np.where(w > 0, img, np.float32(0)))
    other = case("d_tile_edges")[0][::-1].copy()
    w2 = content_based_weights(other, s1, s2)
    got2 = fuse_weighted_average([img, other], [ident, ident], (0, 0, 0), dims, use_blending=False,
                                 use_content_based=True, content_sigma1=s1, content_sigma2=s2)
    a, b = w.astype(np.float64), w2.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        want2 = np.where(a + b > 0, (img * a + other * b) / (a + b), 0.0).astype(np.float32)
    np.testing.assert_array_equal(got2, want2)


def staged(img, on_device):
    """a private copy of img where the call shall find it, and its address"""
    import torch
    a = torch.from_numpy(img.copy()).cuda() if on_device else img.copy()
    torch.cuda.synchronize()   # the library runs on its own stream
    return a, C.c_void_p(a.data_ptr() if on_device else a.ctypes.data)


def test_host_and_device_pointers_give_the_same_bits(gpu, lib):
    import torch
    img, s1, s2, _, _ = case("a_multifold_z")
    host = content_based_weights(img, s1, s2)
    dev = content_based_weights(torch.from_numpy(img.copy()).cuda(), s1, s2)
    assert dev.is_cuda
    np.testing.assert_array_equal(dev.cpu().numpy(), host)
    np.testing.assert_array_equal(content_based_weights(img, s1, s2), host)   # and run to run
    # the C entry with every pairing of a host / device-resident image and result
    img, s1, s2, w64, w32 = case("s_staging")
    host = content_based_weights(img, s1, s2)
    check_against_restatement("s_staging", host, w64, w32)
    dims = (C.c_int64 * 3)(*img.shape[::-1])
    sig = [(C.c_double * 3)(*s) for s in (s1, s2)]
    for src_dev in (False, True):
        for out_dev in (False, True):
            src, sp = staged(img, src_dev)
            out, op = staged(np.zeros_like(img), out_dev)
            assert lib.spim_content_based_weights(sp, dims, sig[0], sig[1], op, 0) == 0
            got = out.cpu().numpy() if out_dev else out
            np.testing.assert_array_equal(got.view(np.uint32), host.view(np.uint32), err_msg=f"{src_dev} {out_dev}")
            np.testing.assert_array_equal(src.cpu().numpy() if src_dev else src, img)   # the image is only read


def test_old_entry_point_is_unchanged(gpu):
    """fuse_weighted_average without content-based weights, as C1 checks it, small."""
    srcs, models, bb_min, bb_dims, borders, ranges, _, _, _, _ = fusion_inputs()
    for blend in (True, False):
        got = fuse_weighted_average(srcs, models, bb_min, bb_dims, 1.0, 1, blend, borders, ranges)
        want = fr.fuse_weighted_average(srcs, models, bb_min, bb_dims, 1.0, 1, blend, borders, ranges)
        assert (want > 0).mean() > 0.3 and (want == 0).any()
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-4)


def test_bad_arguments(gpu, lib):
    img = np.ones((4, 5, 6), np.float32)
    out = np.empty_like(img)
    dims = (C.c_int64 * 3)(6, 5, 4)
    good = (C.c_double * 3)(2, 2, 2)
    call = lib.spim_content_based_weights
    assert call(img.ctypes.data, dims, good, good, out.ctypes.data, 0) == 0
    for bad in ((0.0, 2, 2), (2, -1.0, 2), (2, 2, math.nan), (math.inf, 2, 2), (2, 1e9, 2)):
        b = (C.c_double * 3)(*bad)
        assert call(img.ctypes.data, dims, b, good, out.ctypes.data, 0) == ERR_ARG
        assert "sigma" in _lib.last_error()
        assert call(img.ctypes.data, dims, good, b, out.ctypes.data, 0) == ERR_ARG
    assert call(None, dims, good, good, out.ctypes.data, 0) == ERR_ARG
    assert "null" in _lib.last_error()
    assert call(img.ctypes.data, None, good, good, out.ctypes.data, 0) == ERR_ARG
    assert call(img.ctypes.data, dims, None, good, out.ctypes.data, 0) == ERR_ARG
    assert call(img.ctypes.data, dims, good, None, out.ctypes.data, 0) == ERR_ARG
    assert call(img.ctypes.data, dims, good, good, None, 0) == ERR_ARG
    with pytest.raises(_lib.SpimDeconError):
        content_based_weights(img, (2, 2, 0), (3, 3, 3))
    # the fusion call
    view = (_lib.ViewSource * 1)()
    view[0].img = _lib.fptr(img)
    view[0].dims[:] = [6, 5, 4]
    view[0].model[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    p = _lib.FusionParams()
    lib.spim_fusion_params_default(C.byref(p))
    p.bb_dims[:] = [6, 5, 4]
    p.use_blending = 0
    fuse = lib.spim_fuse_weighted_average_content
    assert fuse(1, view, C.byref(p), None, None, good, good, _lib.fptr(out)) == 0
    assert fuse(1, view, C.byref(p), None, None, None, good, _lib.fptr(out)) == ERR_ARG
    assert fuse(1, view, C.byref(p), None, None, good, None, _lib.fptr(out)) == ERR_ARG
    assert fuse(1, view, C.byref(p), None, None, good, (C.c_double * 3)(2, 0, 2), _lib.fptr(out)) == ERR_ARG
    assert fuse(1, view, C.byref(p), None, None, good, good, None) == ERR_ARG
    p.use_blending = 1
    assert fuse(1, view, C.byref(p), None, None, good, good, _lib.fptr(out)) == ERR_ARG   # no borders
