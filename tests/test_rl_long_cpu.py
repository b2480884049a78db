"""CPU: the premises of tests/test_gpu_rl_long.py, on the oracle alone.

That module runs RL at the BASELINE configs' own iteration counts, bounds what fp16
storage costs against the fp32 reference, and gives the views of one session kernels of
different sizes.  Its bounds rest on four facts about the oracle that need no GPU:

- the float32-FFT oracle, the yardstick of the per-voxel bound, stays within 1e-4
  relative L2 of the float64 oracle at every checkpoint of every long case (measured
  1e-7 .. 5e-7), so "MAXNORM_K x the f32 oracle's error" is a bound far inside 1e-4;
- rounding img and weight to fp16 moves the float64 oracle's psi by more than 1e-5 and
  zeroes no weight, so the fp16 cases can see the rounding and their masks are equal;
- zero-padding the kernels of a mixed-size session to a common size gives a different
  psi (> 1e-3: the normImg portions and the "same"-size crop of the compound kernels
  follow each kernel's own dims), so the session must place each kernel in its own dims;
- placing one view's prepared kernels one voxel off centre moves psi by more than 1e-2,
  100 times the GPU tests' bound.

This file also holds what both modules share: the long cases, the mixed kernel sizes and
the oracle run that keeps psi at the checkpoints (``trace``).
"""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from oracle import mvdecon_ref as ref
from test_asym_cpu import asym_psf, test_asymmetric_psf_is_non_degenerate as check_psf
from test_gpu_asym_psf import case, key_of, max_err

PSFTYPE = ref.PSFTYPE


class Long:
    """One BASELINE config's rule (PSFTYPE, lambda, views, iterations) on the smallest
    volume of the fast engine passes: x = 248 + 8 pads to 256, the shortest two-factor
    x-tile row, and nx % 4 == 0; 9^3 PSFs; z runs the direct pass at any length."""

    def __init__(self, shape, V, cid, psftype, lam, iters, fp16=False):
        self.key = key_of(shape, (9, 9, 9), V=V, cid=cid, fp16=fp16)
        self.shape, self.psftype, self.lam, self.iters, self.fp16 = shape, psftype, lam, iters, fp16
        self.checkpoints = tuple(n for n in (1, 5, 10, 20) if n <= iters)


# ny = 40: the smallest ny > nz that 8 y-slabs of >= cy + 1 = 5 rows divide.  BASELINE.json
# states no iteration count for config 5; it runs config 2's 10 here.
LONG = {
    "c2": Long((7, 24, 248), 4, 62, PSFTYPE.INDEPENDENT, 0.0, 10),
    "c3": Long((7, 40, 248), 6, 63, PSFTYPE.EFFICIENT_BAYESIAN, 0.006, 20),
    "c5": Long((7, 40, 248), 6, 65, PSFTYPE.OPTIMIZATION_I, 0.006, 10, fp16=True),
}

# the short fp16 case: test_gpu_rl.test_fp16_storage's shape, rule and 4 iterations
FP16_SHORT = dict(shape=(20, 24, 28), ksize=(7, 9, 11), V=2, cid=7, partial=False,
                  psftype=PSFTYPE.OPTIMIZATION_I, lam=0.006, iters=4)

# per-view kernel sizes (kx, ky, kz): they differ on every axis and no view is the largest
# on all three, so the session's halo is a mix of views
MIXED3 = ((7, 9, 11), (11, 5, 7), (5, 11, 9))
MIXED_SETS = {
    "rl": MIXED3,
    "z 2cz+1": ((9, 5, 7), (5, 7, 3)),
    "z 540": ((3, 5, 25), (5, 3, 17)),
    "trim small first": ((5, 3, 17), (3, 5, 23)),
    "trim large first": ((3, 5, 23), (5, 3, 17)),
    "trim off": ((3, 5, 25), (5, 3, 23)),
    "x 540": ((9, 7, 3), (21, 3, 5)),
    "y 540": ((5, 25, 3), (3, 9, 5)),
    "pad": ((5, 7, 3), (3, 5, 7)),
    "z slabs": ((5, 7, 9), (9, 5, 3)),
    "y split": ((9, 7, 5), (5, 3, 9), (7, 9, 3)),
    "device groups": ((9, 7, 5), (5, 5, 9)),
    "golden rl_mixed_ksize": ((5, 7, 9), (9, 3, 5), (3, 9, 7)),
}


class Trace:
    pass


@functools.lru_cache(maxsize=None)
def trace(key, psftype, iters, lam, checkpoints, precision="f64"):
    """ref.mv_deconvolution run once, keeping psi (before the mask) after each of
    ``checkpoints`` iterations: .psi[n], .stats [iteration][view], .count, .avg, .final."""
    imgs, ws, ks = case(*key)
    k1, k2 = ref.prepare_kernels(ks, psftype, 8)
    t = Trace()
    t.count, t.avg = ref.first_iteration(imgs)
    psi = np.full(imgs[0].shape, np.float32(t.avg), np.float32)
    t.psi, t.stats = {}, []
    for n in range(1, iters + 1):
        psi, st = ref.run_iteration(psi, imgs, ws, k1, k2, lam, precision)
        t.stats.append(st)
        if n in checkpoints:
            psi.setflags(write=False)
            t.psi[n] = psi
    t.final = np.where(t.count == 0, np.float32(0.0), psi).astype(np.float32)
    t.final.setflags(write=False)
    t.stats = np.array(t.stats)
    return t


def long_traces(name):
    c = LONG[name]
    args = (c.key, c.psftype, c.iters, c.lam, c.checkpoints)
    return trace(*args), trace(*args, precision="f32")


def unrounded(key):
    return key[:6] + (False,)


# ------------------------------------------------------------------ the kernels

@pytest.mark.parametrize("V", [4, 6])
def test_long_case_psfs_are_non_degenerate(V):
    for v in range(V):
        check_psf(v, V, (9, 9, 9))


@pytest.mark.parametrize("name", list(MIXED_SETS))
def test_mixed_sizes_differ_and_share_the_halo(name):
    sizes = MIXED_SETS[name]
    for v, size in enumerate(sizes):
        check_psf(v, len(sizes), size)
    big = [max(s[d] for s in sizes) for d in range(3)]
    assert all(tuple(s) != tuple(big) for s in sizes)         # no view is the largest on every axis
    for d in range(3):
        assert len({s[d] for s in sizes}) > 1, d              # the sizes differ on every axis


# ------------------------------------------------------------------ A: the yardstick

@pytest.mark.parametrize("name", list(LONG))
def test_f32_oracle_stays_on_f64_oracle(name):
    t64, t32 = long_traces(name)
    cov = t64.count > 0
    for n in LONG[name].checkpoints:
        e = rel_l2(t32.psi[n][cov], t64.psi[n][cov])
        print(f"\n{name} n={n}: f32 oracle rel_l2 {e:.2e} max {max_err(t32.psi[n][cov], t64.psi[n][cov]):.2e}")
        assert e < 1e-4, (n, e)
    assert np.array_equal(t32.final == 0, t64.final == 0)
    np.testing.assert_allclose(t32.stats[:, :, 0], t64.stats[:, :, 0], rtol=1e-3)


# ------------------------------------------------------------------ B: the rounding cost

def fp16_keys():
    s = FP16_SHORT
    short = key_of(s["shape"], s["ksize"], V=s["V"], cid=s["cid"], partial=s["partial"], fp16=True)
    return {"c5": (LONG["c5"].key, LONG["c5"].psftype, LONG["c5"].iters, LONG["c5"].lam),
            "short": (short, s["psftype"], s["iters"], s["lam"])}


def fp16_oracles(name):
    """(O16, O32, max-norm error of the f32 oracle on the rounded inputs): the float64
    oracle's masked psi on the fp16-rounded and on the fp32 inputs."""
    key, pt, iters, lam = fp16_keys()[name]
    cps = LONG["c5"].checkpoints if name == "c5" else (iters,)      # (the cached run of section A)
    o16 = trace(key, pt, iters, lam, cps).final
    return o16, trace(unrounded(key), pt, iters, lam, cps).final, max_err(trace(key, pt, iters, lam, cps, "f32").final, o16)


@pytest.mark.parametrize("name", ["c5", "short"])
def test_fp16_rounding_is_visible_and_zeroes_no_weight(name):
    key, pt, iters, lam = fp16_keys()[name]
    o16, o32 = fp16_oracles(name)[:2]
    e = rel_l2(o16, o32)
    print(f"\n{name}: E_round rel_l2 {e:.3e} max {max_err(o16, o32):.3e}")
    assert e > 1e-5, e
    assert np.array_equal(o16 == 0, o32 == 0)
    for w16, w32 in zip(case(*key)[1], case(*unrounded(key))[1]):
        assert np.array_equal(w16 == 0, w32 == 0)


# ------------------------------------------------------------------ C: kernels in their own dims

SHAPE, ITERS, LAM = (20, 24, 28), 5, 0.006


def embed(k, dims, shift=(0, 0, 0)):
    """k centred in zeros of ``dims``, moved by ``shift`` voxels (z, y, x)."""
    out = np.zeros(dims, np.float32)
    o = [(D - d) // 2 + s for D, d, s in zip(dims, k.shape, shift)]
    out[o[0]:o[0] + k.shape[0], o[1]:o[1] + k.shape[1], o[2]:o[2] + k.shape[2]] = k
    return out


@pytest.fixture(scope="module")
def mixed_rl():
    imgs, ws, ks = case(*key_of(SHAPE, MIXED3, V=3))
    res = ref.mv_deconvolution(imgs, ws, ks, PSFTYPE.OPTIMIZATION_I, ITERS, LAM)
    return imgs, ws, ks, res.psi


def test_padding_kernels_to_a_common_size_changes_psi(mixed_rl):
    imgs, ws, ks, psi = mixed_rl
    big = tuple(max(k.shape[d] for k in ks) for d in range(3))
    padded = [embed(k, big) for k in ks]
    moved = rel_l2(ref.mv_deconvolution(imgs, ws, padded, PSFTYPE.OPTIMIZATION_I, ITERS, LAM).psi, psi)
    print(f"\npadded to {big}: {moved:.3e}")
    assert moved > 1e-3, moved
    # placed after the preparation, in each kernel's own dims, the zeros change nothing
    k1, k2 = ref.prepare_kernels(ks, PSFTYPE.OPTIMIZATION_I, 8)
    same = ref.mv_deconvolution(imgs, ws, None, PSFTYPE.OPTIMIZATION_I, ITERS, LAM,
                                prepared=([embed(k, big) for k in k1], [embed(k, big) for k in k2])).psi
    assert rel_l2(same, psi) < 1e-6


@pytest.mark.parametrize("view", [0, 1, 2])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_voxel_shift_of_one_kernel_moves_psi(mixed_rl, view, axis):
    imgs, ws, ks, psi = mixed_rl
    k1, k2 = ref.prepare_kernels(ks, PSFTYPE.OPTIMIZATION_I, 8)
    shift = tuple(int(d == axis) for d in range(3))
    for which in (0, 1):
        p1, p2 = list(k1), list(k2)
        k = (p1, p2)[which][view]
        (p1, p2)[which][view] = embed(k, tuple(d + 2 for d in k.shape), shift)
        moved = rel_l2(ref.mv_deconvolution(imgs, ws, None, PSFTYPE.OPTIMIZATION_I, ITERS, LAM,
                                            prepared=(p1, p2)).psi, psi)
        print(f"\nview {view} K{which + 1} axis {axis}: {moved:.3e}")
        assert moved > 1e-2, moved
