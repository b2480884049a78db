"""GPU: RL at the configs' own iteration counts, the cost of fp16 storage against the fp32
reference, and views with kernels of different sizes in one session.

A. The other parity tests stop at 5 iterations of the oracle; the 20-iteration config
   tests compare the engine with the rocFFT backend, which shares rl_math.hpp, the kernel
   preparation and the quotient rule with it.  Here the rule of each BASELINE config that
   runs RL (PSFTYPE, lambda, views, iterations) runs on the smallest volume of the fast
   engine passes against the float64 oracle: psi at checkpoints taken by successive
   ``run`` calls on the resident psi, the statistics of every iteration, and the per-voxel
   bound at every checkpoint, so that the error may grow no faster than the float32
   oracle's own.
B. ``storage_fp16`` is compared with the oracle on the fp16-rounded inputs everywhere
   else.  Here it is bounded against the oracle on the fp32 inputs: the rounding cost
   E_round = rel_l2(O16, O32) is a figure of the oracle alone, and the bounds follow
   from the triangle inequality and the bounds on the rounded inputs.
C. Every other session gives all its views one kernel size.  Here the sizes differ on
   every axis and no view is the largest on all three: the halo is a mix of views, each
   prepared kernel is placed in its own dims into the common frame (full spectra, the
   compact 2 cz + 1 planes, the direct z pass's tap layout and its trim), and a y split
   swaps each kernel's own y and z dims.  tests/test_rl_long_cpu.py shows that padding
   the kernels to a common size on the host is not the same RL, and that one voxel off
   centre moves psi by more than 1e-2.

Bounds, as in tests/test_gpu_asym_psf.py: engine vs the float64 oracle 1e-4 relative L2,
equal zero mask, max-norm error <= MAXNORM_K x the float32-FFT oracle's, engine vs the
rocFFT backend 1e-5.
"""
import numpy as np
import pytest

from conftest import rel_l2
from spim_registration_amd.decon import MVDeconFFT, MVDeconInput, MVDeconvolution, PSFTYPE, Session
from test_gpu_asym_psf import MAXNORM_K, TOL, case, check, key_of, max_err, run
from test_gpu_multidevice import TILE_SHAPE, Y_SHAPE
from test_rl_long_cpu import LONG, MIXED_SETS, fp16_keys, fp16_oracles, long_traces, unrounded

pytestmark = pytest.mark.gpu

# MAXNORM_K (4) holds for the long cases too: the rocFFT backend's error over their
# checkpoints is 0.92 .. 1.45 x the f32 oracle's, and the constant is the smallest power
# of two >= 2 x the largest such ratio (DESIGN.md section 2 lists the ratios; a ratio above
# 2 here would call for a constant of these cases' own)


# ------------------------------------------------------------------ A. the configs' counts

class Out:
    pass


def run_long(name, fp16=None, inputs=None, **kw):
    """The case's rule through one session: psi after each checkpoint (successive ``run``
    calls), the statistics of every iteration, the masked psi and the paths taken."""
    c = LONG[name]
    imgs, ws, ks = case(*(inputs or c.key))
    o = Out()
    with Session(c.shape[::-1], storage_fp16=c.fp16 if fp16 is None else fp16, **kw) as s:
        for i, w, k in zip(imgs, ws, ks):
            s.add_view(i, w, k)
        s.init(c.psftype)
        engine = kw.get("fft_backend", "engine") == "engine"
        o.avg = s.init_psi()
        o.psi, stats, done = {}, [], 0
        for n in c.checkpoints:
            stats.append(s.run(n - done, c.lam))
            done = n
            o.psi[n] = s.get_psi()
        o.stats = np.concatenate(stats)
        s.apply_mask()
        o.final = s.get_psi()
        o.nslab = s.num_slabs()
        o.extent = s.slab_extent(0)
        o.xmodes = [s.xpass_mode(i) for i in range(o.nslab)] if engine else None
        o.zmodes = [s.zpass_mode(i) for i in range(o.nslab)] if engine else None
        o.dims = s.fft_dims()
    return o


def check_long(name, o, roc=None, label=""):
    """Every checkpoint, the final psi and every iteration's statistics on the oracle."""
    c = LONG[name]
    t64, t32 = long_traces(name)
    cov = t64.count > 0
    assert abs(o.avg - t64.avg) <= 1e-12 * abs(t64.avg)
    for n in c.checkpoints + ("final",):
        if n == "final":
            psi, exp, f32, rpsi = o.final, t64.final, t32.final, roc.final if roc else None
            assert np.array_equal(psi == 0, exp == 0)
        else:       # before apply_mask: the voxels some view covers
            psi, exp, f32 = o.psi[n][cov], t64.psi[n][cov], t32.psi[n][cov]
            rpsi = roc.psi[n][cov] if roc else None
        assert np.isfinite(psi).all()
        l2, mx, base = rel_l2(psi, exp), max_err(psi, exp), max_err(f32, exp)
        line = (f"\nMAXNORM long {name}{label} n={n}: f32-oracle {base:.3e} (rel_l2 {rel_l2(f32, exp):.2e}) "
                f"engine {mx:.3e} (x{mx / base:.2f}, rel_l2 {l2:.2e})")
        if roc:
            rmx = max_err(rpsi, exp)
            line += f" rocfft {rmx:.3e} (x{rmx / base:.2f})"
            assert rel_l2(psi, rpsi) < 1e-5, n
        print(line)
        assert l2 < TOL, (n, l2)
        assert mx <= MAXNORM_K * base, (n, mx, base, mx / base)
    assert o.stats.shape == t64.stats.shape
    np.testing.assert_allclose(o.stats[:, :, 0], t64.stats[:, :, 0], rtol=1e-3)
    np.testing.assert_allclose(o.stats[:, :, 1], t64.stats[:, :, 1], rtol=1e-2, atol=1e-6)


def assert_fast(o, slabs=1):
    assert o.nslab == slabs and o.xmodes == [2] * slabs and o.zmodes == [3] * slabs, (o.nslab, o.xmodes, o.zmodes)
    assert o.dims[0] == 256, o.dims


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_config_rule_at_its_iteration_count(gpu, name):
    """C2: INDEPENDENT, lambda 0, 4 views, 10 iterations.  C3: EFFICIENT_BAYESIAN, 0.006,
    6 views, 20 iterations."""
    o = run_long(name)
    assert_fast(o)
    roc = run_long(name, fft_backend="rocfft")
    check_long(name, roc, label=" (rocfft backend)")
    check_long(name, o, roc)


def test_c3_rule_on_eight_y_slabs(gpu):
    """C3's decomposition, 8 device groups (here on one GPU), at its 20 iterations."""
    c = LONG["c3"]
    one = run_long("c3")
    o = run_long("c3", devices=[0] * 8)
    assert_fast(o, 8)
    nz, ny, nx = c.shape
    assert ny > nz and o.extent == (nx, nz, ny // 8), o.extent      # y slabs, kept as (x, z, y) rows
    for n in c.checkpoints:
        assert rel_l2(o.psi[n], one.psi[n]) < 1e-5, n
    assert rel_l2(o.final, one.final) < 1e-5
    np.testing.assert_allclose(o.stats, one.stats, rtol=1e-4)
    check_long("c3", o, label=" 8 y-slabs")


def test_c5_rule_fp16_on_eight_y_slabs(gpu):
    """C5: OPTIMIZATION_I, 0.006, 6 views, fp16 storage, 8 local y-slabs; the oracle runs
    on the fp16-rounded inputs."""
    c = LONG["c5"]
    o = run_long("c5", local_slabs=8)
    assert_fast(o, 8)
    nz, ny, nx = c.shape
    assert o.extent == (nx, nz, ny // 8), o.extent
    roc = run_long("c5", fft_backend="rocfft")
    check_long("c5", roc, label=" (rocfft backend)")
    check_long("c5", o, roc)


# ------------------------------------------------------------------ B. fp16 against fp32 inputs

def run_fp16_on_fp32_inputs(name):
    """psi of a ``storage_fp16`` session that is handed the fp32 inputs."""
    if name == "c5":
        o = run_long("c5", fp16=True, inputs=unrounded(LONG["c5"].key), local_slabs=8)
        assert_fast(o, 8)
        return o.final
    key, pt, iters, lam = fp16_keys()[name]
    imgs, ws, ks = case(*unrounded(key))
    with Session(imgs[0].shape[::-1], storage_fp16=True) as s:
        for i, w, k in zip(imgs, ws, ks):
            s.add_view(i, w, k)
        s.init(pt)
        s.init_psi()
        s.run(iters, lam)
        s.apply_mask()
        return s.get_psi()


@pytest.mark.parametrize("name", ["c5", "short"])
def test_fp16_storage_against_the_fp32_reference(gpu, name):
    """rel_l2(psi16, O32) <= E_round + 1e-4 |O16| / |O32| and max_err(psi16, O32) <=
    max_err(O16, O32) + MAXNORM_K E_f32 max|O16| / max|O32|: the triangle inequality over
    the bounds asserted on the rounded inputs.  Nothing here is taken from the engine."""
    o16, o32, base = fp16_oracles(name)
    psi16 = run_fp16_on_fp32_inputs(name)
    e_round, m_round = rel_l2(o16, o32), max_err(o16, o32)
    n16, n32 = np.linalg.norm(o16.astype(np.float64)), np.linalg.norm(o32.astype(np.float64))
    l2, mx = rel_l2(psi16, o32), max_err(psi16, o32)
    print(f"\nFP16COST {name}: E_round {e_round:.3e} (max {m_round:.3e}) engine vs fp32 reference {l2:.3e} "
          f"(max {mx:.3e}); vs rounded-input oracle {rel_l2(psi16, o16):.2e}")
    assert e_round > 1e-5, e_round
    assert np.isfinite(psi16).all()
    assert np.array_equal(psi16 == 0, o32 == 0)
    assert l2 <= e_round + TOL * n16 / n32, (l2, e_round)
    assert mx <= m_round + MAXNORM_K * base * float(np.max(np.abs(o16)) / np.max(np.abs(o32))), (mx, m_round, base)


# ------------------------------------------------------------------ C. per-view kernel sizes

def mixed_key(name, shape, **kw):
    sizes = MIXED_SETS[name]
    return key_of(shape, sizes, V=len(sizes), **kw)


@pytest.mark.parametrize("psftype,lam,weights,partial", [
    (PSFTYPE.INDEPENDENT, 0.0, "ones", False),
    (PSFTYPE.INDEPENDENT, 0.006, "blend", False),
    (PSFTYPE.OPTIMIZATION_I, 0.006, "blend", True),
    (PSFTYPE.OPTIMIZATION_II, 0.0, "blend", False),
    (PSFTYPE.EFFICIENT_BAYESIAN, 0.006, "blend", True),
])
def test_mvdeconvolution_mixed_sizes(gpu, psftype, lam, weights, partial):
    """The compound kernels are "same"-size in each view's own dims."""
    key = mixed_key("rl", (20, 24, 28), weights=weights, partial=partial)
    imgs, ws, ks = case(*key)
    inp = MVDeconInput()
    for i, w, k in zip(imgs, ws, ks):
        inp.add(MVDeconFFT(i, w, k, device_list=[0]))
    dec = MVDeconvolution(inp, psftype, 5, lam, ij_threads=8)
    roc = run(key, psftype, 5, lam, fft_backend="rocfft")
    assert rel_l2(dec.get_psi(), roc.psi) < 1e-5
    res = check(f"mixed rl {psftype.name} lam={lam}", dec.get_psi(), key, psftype, 5, lam, rocfft=roc.psi)
    st = np.array(res.stats)
    np.testing.assert_allclose(dec.stats[:, :, 0], st[:, :, 0], rtol=1e-3)
    np.testing.assert_allclose(dec.stats[:, :, 1], st[:, :, 1], rtol=1e-2, atol=1e-6)
    assert abs(dec.avg - res.avg) <= 1e-12 * abs(res.avg)


@pytest.mark.parametrize("name,shape", [("z 2cz+1", (40, 18, 22)), ("z 540", (516, 10, 12))])
def test_z_pass_modes_mixed_sizes(gpu, name, shape, monkeypatch):
    """Direct z convolution (mode 3), compact-kernel FFT z pass (1), full spectra (0): the
    smaller kernel sits inside the 2 cz + 1 planes of the larger."""
    key = mixed_key(name, shape)
    out = []
    for zk, zd, mode in (("compact", "1", 3), ("compact", "0", 1), ("full", "1", 0)):
        monkeypatch.setenv("SPIMDECON_ZK", zk)
        monkeypatch.setenv("SPIMDECON_ZDIRECT", zd)
        o = run(key, fft_pad_policy="fast")
        assert o.zmode == mode
        out.append(o.psi)
    if name == "z 540":
        assert o.dims[2] == 540, o.dims
    roc = run(key, fft_backend="rocfft")
    assert not np.array_equal(out[0], out[2]), "direct path not taken (identical bits)"
    assert not np.array_equal(out[1], out[2]), "compact FFT path not taken (identical bits)"
    assert rel_l2(out[0], out[2]) < 1e-5
    assert rel_l2(out[1], out[2]) < 1e-5
    for psi, path in zip(out, ("direct", "compact-fft", "full")):
        assert rel_l2(psi, roc.psi) < 1e-5
        check(f"mixed {name} {path}", psi, key, rocfft=roc.psi)


@pytest.mark.parametrize("name", ["trim small first", "trim large first", "trim off"])
def test_z_tap_trim_mixed_sizes(gpu, name, monkeypatch):
    """The trim of the KC-12 layout's outer taps follows the common cz: on with 23 planes
    next to 17, in either view order; off with 25 next to 23.  Either way psi has the bits
    of the runtime-masked kernel (SPIMDECON_ZKD=0)."""
    key = mixed_key(name, (200, 10, 12), cid=44)
    out = []
    for zkd in ("1", "0"):
        monkeypatch.setenv("SPIMDECON_ZKD", zkd)
        o = run(key, fft_pad_policy="fast")
        assert o.zmode == 3
        out.append(o.psi)
    assert np.array_equal(out[0], out[1])
    roc = run(key, fft_backend="rocfft")
    assert rel_l2(out[0], roc.psi) < 1e-5
    check(f"mixed {name}", out[0], key, rocfft=roc.psi)


@pytest.mark.parametrize("fp16", [False, True])
def test_x_tiles_540_mixed_sizes(gpu, fp16):
    key = mixed_key("x 540", (12, 24, 516), cid=41, fp16=fp16)
    o = run(key, fft_pad_policy="fast")
    roc = run(key, fft_backend="rocfft")
    assert o.dims[0] == 540 and o.xmode == 2, (o.dims, o.xmode)
    assert rel_l2(o.psi, roc.psi) < 1e-5
    np.testing.assert_allclose(o.stats, roc.stats, rtol=1e-3)
    check(f"mixed x 540{' fp16' if fp16 else ''}", o.psi, key, rocfft=roc.psi)


def test_y_pass_540_mixed_sizes(gpu):
    key = mixed_key("y 540", (10, 500, 12))
    o = run(key, fft_pad_policy="fast")
    roc = run(key, fft_backend="rocfft")
    assert o.dims[1] == 540, o.dims
    assert rel_l2(o.psi, roc.psi) < 1e-5
    check("mixed y 540", o.psi, key, rocfft=roc.psi)


@pytest.mark.parametrize("policy", ["smooth", "fast"])
def test_pad_policies_mixed_sizes(gpu, policy):
    key = mixed_key("pad", (33, 17, 46))
    o = run(key, PSFTYPE.OPTIMIZATION_II, 3, 0.0, fft_pad_policy=policy)
    roc = run(key, PSFTYPE.OPTIMIZATION_II, 3, 0.0, fft_backend="rocfft")
    assert rel_l2(o.psi, roc.psi) < 1e-5, o.dims
    check(f"mixed pad {policy} {o.dims}", o.psi, key, PSFTYPE.OPTIMIZATION_II, 3, 0.0, rocfft=roc.psi)


@pytest.mark.parametrize("slabs", [2, 3])
def test_z_slabs_mixed_sizes(gpu, slabs):
    """The halo of every slab is the largest z size's."""
    key = mixed_key("z slabs", (40, 20, 22))
    one, o = run(key), run(key, local_slabs=slabs, slab_axis="z")
    assert len(o.xmodes) == slabs
    assert rel_l2(o.psi, one.psi) < 1e-5
    np.testing.assert_allclose(o.stats, one.stats, rtol=1e-4)
    check(f"mixed z slabs {slabs}", o.psi, key, rocfft=run(key, fft_backend="rocfft").psi)


def test_y_split_mixed_sizes(gpu):
    """Each kernel's own y and z dims swap; they differ per view and from each other, so a
    missed or doubled swap of one view's dims reads another kernel shape."""
    key = mixed_key("y split", Y_SHAPE, cid=13)
    pt = PSFTYPE.EFFICIENT_BAYESIAN
    z = run(key, pt, local_slabs=1, slab_axis="z")
    y = run(key, pt, local_slabs=2, slab_axis="y")
    assert y.xmodes == [2, 2], y.xmodes
    assert rel_l2(y.psi, z.psi) < 1e-5
    np.testing.assert_allclose(y.stats, z.stats, rtol=1e-4)
    check("mixed y split", y.psi, key, pt, rocfft=run(key, pt, fft_backend="rocfft").psi)


def test_device_groups_mixed_sizes(gpu):
    key = mixed_key("device groups", TILE_SHAPE, cid=11)
    one = run(key)
    o = run(key, devices=[0, 0], local_slabs=2)
    assert o.ndev == 2 and o.xmodes == [2] * 4 and one.xmodes == [2], (o.ndev, o.xmodes)
    assert rel_l2(o.psi, one.psi) < 1e-5
    np.testing.assert_allclose(o.stats, one.stats, rtol=1e-4)
    check("mixed device groups", o.psi, key, rocfft=run(key, fft_backend="rocfft").psi)
