"""GPU: every RL code path with asymmetric, non-separable PSFs (synthetic.psf_asymmetric).

The other GPU tests take their kernels from synthetic.psf, a centred Gaussian: it equals
its own point reflection and its mirror images, and its spectrum is real.  Inverting a
kernel, the order of the taps in a window, the sign of the centre shift, the y/z swap of a
y-split slab and the imaginary part of every packed complex multiply are then invisible
(tests/test_asym_cpu.py measures this on the oracle).  Each case here mirrors one of
those tests -- the same small shape, the same path-selection asserts, the same bounds
(engine vs rocFFT backend 1e-5, engine vs the float64 oracle 1e-4 relative L2) -- with
kernels that have none of these symmetries.

Next to the relative L2 norm, which one wrong voxel, row or corner cannot move, the RL
cases bound the largest voxel error max|psi - oracle| / max|oracle| by MAXNORM_K times
the same figure of the oracle run with float32 FFTs (``precision="f32"``): the error a
correct float32 implementation of the same arithmetic makes on these inputs.  MAXNORM_K
comes from the rocFFT backend, the reference implementation on the GPU, not from the
engine under test ("Tolerances").
"""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from oracle import lrsim_ref, mvdecon_ref as ref
from spim_registration_amd import synthetic
from spim_registration_amd.decon import (MVDeconFFT, MVDeconInput, MVDeconvolution, PSFTYPE,
                                         Session, prepare_kernels)
from spim_registration_amd.lr_multiview import LucyRichardsonFFT, LucyRichardsonMultiViewDeconvolution
from test_asym_cpu import asym_psf
from test_gpu_multidevice import TILE_K, TILE_SHAPE, Y_SHAPE

pytestmark = pytest.mark.gpu

TOL = 1e-4
# smallest power of two >= 2 x the largest (rocFFT backend error / f32-oracle error) over
# the cases of this file: that ratio is 0.40 .. 2.00 (DESIGN.md section 2 lists every case)
MAXNORM_K = 4

OPT1 = PSFTYPE.OPTIMIZATION_I
MIXED_BLUR = (5, 5, 5)     # the common blur of the views of a case with per-view kernel sizes


def max_err(a, b):
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / np.max(np.abs(b)))


@functools.lru_cache(maxsize=None)
def case(shape, ksize, V=2, cid=7, weights="blend", partial=True, fp16=False):
    """Views blurred with the asymmetric kernels (read-only; shared between tests).
    ``ksize``: one (kx, ky, kz) for every view, or a tuple of V of them (per-view kernel
    sizes: the views are blurred with MIXED_BLUR-sized kernels and RL runs with the
    given ones, tests/test_gpu_rl_long.py)."""
    mixed = isinstance(ksize[0], tuple)
    imgs, ws, ks, _ = synthetic.make_views(shape, V, config_id=cid, ksize=MIXED_BLUR if mixed else ksize,
                                           weights=weights, partial=partial, bead_density=1.0 / 6 ** 3,
                                           asymmetric=True)
    sizes = ksize if mixed else (ksize,) * V
    assert len(sizes) == V
    if mixed:
        ks = [asym_psf(v, V, sizes[v]) for v in range(V)]
    for v, k in enumerate(ks):
        assert np.array_equal(k, asym_psf(v, V, sizes[v]))   # the kernels test_asym_cpu.py checks
    if fp16:   # the oracle runs on the fp16-rounded inputs the session stores
        imgs = [i.astype(np.float16).astype(np.float32) for i in imgs]
        ws = [w.astype(np.float16).astype(np.float32) for w in ws]
    for a in imgs + ws + ks:
        a.setflags(write=False)
    return imgs, ws, ks


@functools.lru_cache(maxsize=None)
def oracle(key, psftype=OPT1, iters=3, lam=0.006):
    """(float64 oracle, max-norm error of the float32-FFT oracle against it)."""
    imgs, ws, ks = case(*key)
    res = ref.mv_deconvolution(imgs, ws, ks, psftype, iters, lam)
    r32 = ref.mv_deconvolution(imgs, ws, ks, psftype, iters, lam, precision="f32")
    res.psi.setflags(write=False)
    return res, max_err(r32.psi, res.psi)


class Out:
    pass


def run(key, psftype=OPT1, iters=3, lam=0.006, **kw):
    imgs, ws, ks = case(*key)
    o = Out()
    with Session(imgs[0].shape[::-1], storage_fp16=key[6], **kw) as s:
        for i, w, k in zip(imgs, ws, ks):
            s.add_view(i, w, k)
        s.init(psftype)
        o.zmode = s.zpass_mode() if kw.get("fft_backend", "engine") == "engine" else None
        s.init_psi()
        o.stats = s.run(iters, lam)
        s.apply_mask()
        nslab = s.num_slabs()
        o.xmodes = [s.xpass_mode(i) for i in range(nslab)]
        o.xmode = o.xmodes[0]
        o.dims = s.fft_dims()
        o.ndev = s.num_devices()
        o.psi = s.get_psi()
    return o


def check(name, psi, key, psftype=OPT1, iters=3, lam=0.006, rocfft=None):
    """psi on the oracle: 1e-4 relative L2 and the per-voxel bound.  ``rocfft``: the rocFFT
    backend's psi of the same case, printed for the record of MAXNORM_K."""
    res, base = oracle(key, psftype, iters, lam)
    assert np.isfinite(psi).all()
    l2, mx = rel_l2(psi, res.psi), max_err(psi, res.psi)
    line = f"\nMAXNORM {name}: f32-oracle {base:.3e} engine {mx:.3e} (x{mx / base:.2f}, rel_l2 {l2:.2e})"
    if rocfft is not None:
        rmx = max_err(rocfft, res.psi)
        line += f" rocfft {rmx:.3e} (x{rmx / base:.2f})"
    print(line)
    assert l2 < TOL, l2
    assert ((psi == 0) == (res.psi == 0)).all()
    assert mx <= MAXNORM_K * base, (mx, base, mx / base)
    return res


def key_of(shape, ksize, V=2, cid=7, weights="blend", partial=True, fp16=False):
    return (shape, ksize, V, cid, weights, partial, fp16)


# ------------------------------------------------------------------ a. kernel preparation

def _check_kernels(ks, psftype):
    views = [MVDeconFFT(np.ones((4, 4, 4)), np.ones((4, 4, 4)), k) for k in ks]
    k1, k2 = prepare_kernels(views, psftype, ij_threads=8)
    r1, r2 = ref.prepare_kernels(ks, psftype, 8)
    for a, b in zip(k1, r1):
        assert rel_l2(a, b) < 1e-6
    for a, b in zip(k2, r2):
        assert rel_l2(a, b) < 1e-5
        # the orientation, which a norm could average away
        assert np.unravel_index(np.argmax(a), a.shape) == np.unravel_index(np.argmax(b), b.shape)
        assert rel_l2(a, ref.inverted_kernel(b)) > 0.1       # (the fixture can tell)


@pytest.mark.parametrize("psftype", list(PSFTYPE))
def test_prepare_kernels_asymmetric(gpu, psftype):
    ks = [asym_psf(0, 3, (7, 9, 11)), asym_psf(1, 3, (9, 7, 11)), asym_psf(2, 3, (5, 9, 7))]
    _check_kernels([(k * 3.7).astype(np.float32) for k in ks], psftype)


@pytest.mark.parametrize("psftype", [PSFTYPE.OPTIMIZATION_I, PSFTYPE.OPTIMIZATION_II, PSFTYPE.EFFICIENT_BAYESIAN])
def test_prepare_kernels_large_compound_asymmetric(gpu, psftype):
    """k_conv_same_zero_blk: the taps of each compound-kernel output split over a block."""
    ks = [asym_psf(v, 4, (31, 19, 31)) for v in range(3)] + [asym_psf(3, 4, (25, 19, 21))]
    _check_kernels(ks, psftype)


# ------------------------------------------------------------------ b. whole RL

@pytest.mark.parametrize("psftype,lam,weights,partial", [
    (PSFTYPE.INDEPENDENT, 0.0, "ones", False),
    (PSFTYPE.INDEPENDENT, 0.006, "blend", False),
    (PSFTYPE.OPTIMIZATION_I, 0.006, "blend", True),
    (PSFTYPE.OPTIMIZATION_II, 0.0, "blend", False),
    (PSFTYPE.EFFICIENT_BAYESIAN, 0.006, "blend", True),
])
def test_mvdeconvolution_asymmetric(gpu, psftype, lam, weights, partial):
    key = key_of((20, 24, 28), (7, 9, 11), V=3, weights=weights, partial=partial)
    imgs, ws, ks = case(*key)
    inp = MVDeconInput()
    for i, w, k in zip(imgs, ws, ks):
        inp.add(MVDeconFFT(i, w, k, device_list=[0]))
    dec = MVDeconvolution(inp, psftype, 5, lam, ij_threads=8)
    roc = run(key, psftype, 5, lam, fft_backend="rocfft")
    res = check(f"rl {psftype.name} lam={lam}", dec.get_psi(), key, psftype, 5, lam, rocfft=roc.psi)
    st = np.array(res.stats)
    np.testing.assert_allclose(dec.stats[:, :, 0], st[:, :, 0], rtol=1e-3)
    np.testing.assert_allclose(dec.stats[:, :, 1], st[:, :, 1], rtol=1e-2, atol=1e-6)
    assert abs(dec.avg - res.avg) <= 1e-12 * abs(res.avg)


# ------------------------------------------------------------------ c. z passes

@pytest.mark.parametrize("shape,ksize", [((40, 18, 22), (9, 5, 7)), ((516, 10, 12), (3, 3, 25))])
def test_z_pass_modes_asymmetric(gpu, shape, ksize, monkeypatch):
    """Direct z convolution (mode 3), compact-kernel FFT z pass (1), full spectra (0)."""
    key = key_of(shape, ksize)
    out = []
    for zk, zd, mode in (("compact", "1", 3), ("compact", "0", 1), ("full", "1", 0)):
        monkeypatch.setenv("SPIMDECON_ZK", zk)
        monkeypatch.setenv("SPIMDECON_ZDIRECT", zd)
        o = run(key, fft_pad_policy="fast")
        assert o.zmode == mode
        out.append(o.psi)
    roc = run(key, fft_backend="rocfft")
    assert not np.array_equal(out[0], out[2]), "direct path not taken (identical bits)"
    assert not np.array_equal(out[1], out[2]), "compact FFT path not taken (identical bits)"
    assert rel_l2(out[0], out[2]) < 1e-5
    assert rel_l2(out[1], out[2]) < 1e-5
    for psi, name in zip(out, ("direct", "compact-fft", "full")):
        assert rel_l2(psi, roc.psi) < 1e-5
        check(f"z {shape} {name}", psi, key, rocfft=roc.psi)


@pytest.mark.parametrize("shape,ksize", [((100, 10, 12), (3, 3, 31)),     # 33-tap bound
                                         ((512, 13, 12), (3, 3, 25)),     # 2 chunks, My odd: half tile
                                         ((770, 9, 12), (3, 3, 31))])     # 33 taps, 4 chunks
def test_direct_z_pass_asymmetric(gpu, shape, ksize, monkeypatch):
    key = key_of(shape, ksize)
    out = []
    for zk, mode in (("compact", 3), ("full", 0)):
        monkeypatch.setenv("SPIMDECON_ZK", zk)
        o = run(key, fft_pad_policy="fast")
        assert o.zmode == mode
        out.append(o.psi)
    roc = run(key, fft_backend="rocfft")
    assert not np.array_equal(out[0], out[1]), "direct path not taken (identical bits)"
    assert rel_l2(out[0], out[1]) < 1e-5
    assert rel_l2(out[0], roc.psi) < 1e-5
    check(f"zd {shape}", out[0], key, rocfft=roc.psi)


def test_z_tap_trim_asymmetric(gpu, monkeypatch):
    """23 planes in the KC-12 layout: the trimmed outer taps are the window's first and
    last, which a reversed window would exchange for live ones."""
    key = key_of((200, 10, 12), (3, 3, 23), cid=44)
    out = []
    for zkd in ("1", "0"):
        monkeypatch.setenv("SPIMDECON_ZKD", zkd)
        o = run(key, fft_pad_policy="fast")
        assert o.zmode == 3
        out.append(o.psi)
    assert np.array_equal(out[0], out[1])
    roc = run(key, fft_backend="rocfft")
    assert rel_l2(out[0], roc.psi) < 1e-5
    check("z tap trim", out[0], key, rocfft=roc.psi)


def test_thin_volume_asymmetric(gpu):
    key = key_of((1, 16, 20), (5, 5, 3))
    o, roc = run(key), run(key, fft_backend="rocfft")
    assert rel_l2(o.psi, roc.psi) < 1e-5
    check("thin", o.psi, key, rocfft=roc.psi)


# ------------------------------------------------------------------ d. x tiles

@pytest.mark.parametrize("shape,ksize,lx,fp16", [((12, 24, 516), (9, 9, 9), 540, False),
                                                 ((10, 16, 1024), (9, 9, 9), 1050, False),    # TR 64
                                                 ((10, 12, 2048), (21, 3, 3), 2100, False),   # wave tiles
                                                 ((10, 12, 2048), (21, 3, 3), 2100, True),
                                                 ((6, 10, 360), (25, 5, 3), 384, False)])     # global twiddles
def test_x_tiles_asymmetric(gpu, shape, ksize, lx, fp16):
    key = key_of(shape, ksize, cid=41, fp16=fp16)
    o = run(key, fft_pad_policy="fast")
    roc = run(key, fft_backend="rocfft")
    assert o.dims[0] == lx and o.xmode == 2, (o.dims, o.xmode)
    assert rel_l2(o.psi, roc.psi) < 1e-5
    np.testing.assert_allclose(o.stats, roc.stats, rtol=1e-3)
    check(f"x {lx}{' fp16' if fp16 else ''}", o.psi, key, rocfft=roc.psi)


# ------------------------------------------------------------------ e. y passes

def test_y_pass_540_asymmetric(gpu):
    key = key_of((10, 500, 12), (3, 25, 3))
    o = run(key, fft_pad_policy="fast")
    roc = run(key, fft_backend="rocfft")
    assert o.dims[1] == 540, o.dims
    assert rel_l2(o.psi, roc.psi) < 1e-5
    check("y 540", o.psi, key, rocfft=roc.psi)


def test_y_pass_800_prefetch_asymmetric(gpu, monkeypatch):
    """8-column y tiles of 800-point columns; the register prefetch computes the same bits."""
    key = key_of((20, 776, 12), (3, 25, 3))
    out = []
    for ypf in ("1", "0"):
        monkeypatch.setenv("SPIMDECON_YPF", ypf)
        o = run(key, fft_pad_policy="fast")
        assert o.dims[1] == 800 and o.zmode == 3, (o.dims, o.zmode)
        out.append(o.psi)
    assert np.array_equal(out[0], out[1])
    roc = run(key, fft_backend="rocfft")
    assert rel_l2(out[0], roc.psi) < 1e-5
    check("y 800", out[0], key, rocfft=roc.psi)


# ------------------------------------------------------------------ f. Stockham passes

@pytest.mark.parametrize("policy", ["smooth", "fast"])
def test_pad_policies_asymmetric(gpu, policy):
    key = key_of((33, 17, 46), (5, 7, 3))
    o = run(key, PSFTYPE.OPTIMIZATION_II, 3, 0.0, fft_pad_policy=policy)
    roc = run(key, PSFTYPE.OPTIMIZATION_II, 3, 0.0, fft_backend="rocfft")
    assert rel_l2(o.psi, roc.psi) < 1e-5, o.dims
    check(f"pad {policy} {o.dims}", o.psi, key, PSFTYPE.OPTIMIZATION_II, 3, 0.0, rocfft=roc.psi)


# ------------------------------------------------------------------ g. slabs

@pytest.mark.parametrize("slabs", [2, 3])
def test_z_slabs_asymmetric(gpu, slabs):
    key = key_of((40, 20, 22), (5, 7, 9))
    one, o = run(key), run(key, local_slabs=slabs)
    assert rel_l2(o.psi, one.psi) < 1e-5
    np.testing.assert_allclose(o.stats, one.stats, rtol=1e-4)
    check(f"z slabs {slabs}", o.psi, key, rocfft=run(key, fft_backend="rocfft").psi)


@pytest.mark.parametrize("fp16", [False, True])
def test_y_split_asymmetric(gpu, fp16):
    """The session keeps (x, z, y) rows for a y split: the kernel's y and z axes swap."""
    key = key_of(Y_SHAPE, (9, 7, 5), V=3, cid=13, fp16=fp16)
    pt = PSFTYPE.EFFICIENT_BAYESIAN
    z = run(key, pt, local_slabs=1, slab_axis="z")
    y = run(key, pt, local_slabs=2, slab_axis="y")
    assert y.xmodes == [2, 2], y.xmodes
    assert rel_l2(y.psi, z.psi) < 1e-5
    np.testing.assert_allclose(y.stats, z.stats, rtol=1e-4)
    check(f"y split{' fp16' if fp16 else ''}", y.psi, key, pt, rocfft=run(key, pt, fft_backend="rocfft").psi)


def test_device_groups_asymmetric(gpu):
    """Two device groups of two slabs on one GPU (repeated ids: the multi-device code)."""
    key = key_of(TILE_SHAPE, TILE_K, cid=11)
    one = run(key)
    o = run(key, devices=[0, 0], local_slabs=2)
    assert o.ndev == 2 and o.xmodes == [2] * 4 and one.xmodes == [2], (o.ndev, o.xmodes)
    assert rel_l2(o.psi, one.psi) < 1e-5
    np.testing.assert_allclose(o.stats, one.stats, rtol=1e-4)
    check("device groups", o.psi, key, rocfft=run(key, fft_backend="rocfft").psi)


# ------------------------------------------------------------------ h. legacy simultaneous mode

@pytest.mark.parametrize("mult,lam", [(False, 0.0), (True, 0.0), (False, 0.006), (True, 0.006)])
def test_lrsim_asymmetric(gpu, mult, lam):
    sizes = [(7, 9, 11), (9, 7, 5), (5, 5, 9)]
    imgs, ws, _, _ = synthetic.make_views((40, 36, 44), 3, config_id=41, ksize=(9, 9, 9), bead_density=1.0 / 6 ** 3)
    psfs = [asym_psf(v, 3, sizes[v]) * np.float32(3.0) for v in range(3)]       # un-normalised
    exp, avg0, st0 = lrsim_ref.lucy_richardson_multi_view(imgs, ws, psfs, 3, mult, lam)
    stats, avg = [], []
    data = [LucyRichardsonFFT(i, w, k) for i, w, k in zip(imgs, ws, psfs)]
    psi = LucyRichardsonMultiViewDeconvolution.lucyRichardsonMultiView(data, 1, 3, mult, lam, 4, device=gpu,
                                                                       stats_out=stats, avg_out=avg)
    assert avg[0] == pytest.approx(avg0, rel=1e-12)
    err = rel_l2(psi, exp)
    assert err < TOL, err
    np.testing.assert_allclose(np.array(stats), np.array(st0), rtol=1e-3)
