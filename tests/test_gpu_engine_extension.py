"""GPU: the RL engine without its z-extension planes ("extension planes").

A slab without neighbours no longer computes the planes [nz, Mz) of its two spectrum
buffers: the update side reads the planes they mirror (SPIMDECON_EXT_C1), the quotient side
keeps the constant planes a first whole pass left in place (SPIMDECON_EXT_C2).  Every case
runs with both switches on and with both off (the passes as they were) and asks for the
same bits, psi and statistics alike, and for the float64 oracle within the RL tolerance of
the other GPU tests (1e-4 relative L2, the same voxels zero).  Every run must take the x
tiles (xpass_mode 2) and the direct z pass (zpass_mode 3): a shape that falls back fails.

x is padded to 256, the shortest length the x tiles take, and so is y where the rows are
the subject; the kernels are the asymmetric ones of tests/test_gpu_asym_psf.py.  Shapes are
[z, y, x], kernels (kx, ky, kz).
"""
import numpy as np
import pytest

from conftest import rel_l2
from spim_registration_amd.decon import PSFTYPE, Session
from test_gpu_asym_psf import case, key_of, oracle
from test_gpu_multidevice import Y_SHAPE

pytestmark = pytest.mark.gpu

TOL = 1e-4
OPT1 = PSFTYPE.OPTIMIZATION_I
INDEP = PSFTYPE.INDEPENDENT
SWITCHES = ("SPIMDECON_EXT_C1", "SPIMDECON_EXT_C2")


def session_run(key, steps, monkeypatch, on, **kw):
    """``steps``: a list of ("init", psftype) / ("run", iters, lam).  Returns the psi (masked)
    and the statistics after every run step."""
    for name in SWITCHES:
        monkeypatch.setenv(name, "1" if on else "0")
    imgs, ws, ks = case(*key)
    out = []
    with Session(imgs[0].shape[::-1], storage_fp16=key[6], fft_pad_policy="fast", **kw) as s:
        for i, w, k in zip(imgs, ws, ks):
            s.add_view(i, w, k)
        for step in steps:
            if step[0] == "init":
                s.init(step[1])
                s.init_psi()
                n = s.num_slabs()
                dims = [s.fft_dims(i) for i in range(n)]
                assert all(d[0] == 256 for d in dims), dims
                assert [s.zpass_mode(i) for i in range(n)] == [3] * n, dims
                continue
            stats = s.run(step[1], step[2])
            assert [s.xpass_mode(i) for i in range(s.num_slabs())] == [2] * s.num_slabs()
            out.append((s.get_psi(), stats))
        s.apply_mask()
        out.append((s.get_psi(), None))
    return out


def both(key, steps, monkeypatch, **kw):
    """The steps with the switches on and off: the same bits; returns the run with them on."""
    a = session_run(key, steps, monkeypatch, True, **kw)
    b = session_run(key, steps, monkeypatch, False, **kw)
    assert len(a) == len(b)
    for (pa, sa), (pb, sb) in zip(a, b):
        assert np.array_equal(pa, pb)
        assert sa is None or np.array_equal(sa, sb)
    return a


def on_oracle(name, psi, key, psftype, iters, lam):
    res, _ = oracle(key, psftype, iters, lam)
    l2 = rel_l2(psi, res.psi)
    print(f"\nEXT {name}: rel_l2 {l2:.2e}")
    assert np.isfinite(psi).all()
    assert l2 < TOL, l2
    assert ((psi == 0) == (res.psi == 0)).all()
    return res


def single(name, key, psftype, iters, lam, monkeypatch, **kw):
    out = both(key, [("init", psftype), ("run", iters, lam)], monkeypatch, **kw)
    res = on_oracle(name, out[-1][0], key, psftype, iters, lam)
    st = np.array(res.stats)
    np.testing.assert_allclose(out[0][1][:, :, 0], st[:, :, 0], rtol=1e-3)
    return out


@pytest.mark.parametrize("ny", [245, 244])
def test_odd_and_even_rows(gpu, ny, monkeypatch):
    """7 rows of kernel in y: 3 mirror rows per side of an odd or even number of image rows,
    so a row pair holds the last image row and the first extension row when ny is odd."""
    single(f"ny {ny}", key_of((10, ny, 248), (5, 7, 3), cid=23), OPT1, 2, 0.0, monkeypatch)


@pytest.mark.parametrize("shape,ksize,lam,fp16", [
    ((4, 20, 248), (5, 5, 3), 0.0, False),          # nz = 2 cz + 2, 3 planes of kernel
    ((34, 20, 248), (3, 3, 33), 0.006, True),       # nz = 2 cz + 2, 33 planes
    ((260, 20, 248), (3, 5, 3), 0.006, True),       # two z chunks of 130 planes, 4-tap bound
    ((250, 18, 248), (3, 3, 33), 0.0, False),       # two z chunks of 125 planes, 16-tap bound
])
def test_thin_and_chunked_z(gpu, shape, ksize, lam, fp16, monkeypatch):
    """The direct z pass at its limits: the thinnest slab for its taps, where every chunk
    window is mostly mirrored planes, and two chunks, whose carried window head and mirrored
    tail planes meet."""
    single(f"z {shape[0]} k{ksize[2]}", key_of(shape, ksize, cid=29, fp16=fp16), INDEP, 2, lam, monkeypatch)


@pytest.mark.parametrize("slabs,axis,shape", [(2, "z", (40, 20, 248)), (3, "z", (40, 20, 248)), (2, "y", Y_SHAPE)])
def test_slabs_keep_their_planes(gpu, slabs, axis, shape, monkeypatch):
    """Slabs with neighbours hold exchanged halo planes where a lone slab has its extension:
    they must run every pass whole, whatever the switches say."""
    key = key_of(shape, (5, 7, 9), cid=31)
    out = single(f"{slabs} {axis} slabs", key, OPT1, 2, 0.006, monkeypatch, local_slabs=slabs, slab_axis=axis)
    one = session_run(key, [("init", OPT1), ("run", 2, 0.006)], monkeypatch, True)
    assert rel_l2(out[-1][0], one[-1][0]) < 1e-5


def test_second_run_and_new_kernels(gpu, monkeypatch):
    """What a first pass leaves in place must still be there for a second run, and must be
    made anew after an init with other kernels (the spectrum buffers are allocated again)."""
    key = key_of((12, 21, 248), (5, 7, 5), cid=37)
    out = both(key, [("init", OPT1), ("run", 2, 0.006), ("run", 1, 0.006)], monkeypatch)
    on_oracle("run + run", out[-1][0], key, OPT1, 3, 0.006)
    bayes = PSFTYPE.EFFICIENT_BAYESIAN
    out = both(key, [("init", OPT1), ("run", 1, 0.006), ("init", bayes), ("run", 2, 0.0)], monkeypatch)
    on_oracle("new kernels", out[-1][0], key, bayes, 2, 0.0)
