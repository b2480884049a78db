"""GPU: csrc/lrsim.hip at its edges -- the cases of tests/lrsim_cases.py (whose premises
tests/test_lrsim_premises_cpu.py proves) against oracle/lrsim_ref.py, and the update rule
voxel by voxel through lrsim_update_rule.

Tolerances are those of tests/test_gpu_lrsim.py: 1e-4 relative L2 on psi (float FFTs
against the oracle's float64 convolutions), statistics to 1e-3, the initial average to
1e-12, device groups against one group to 1e-6; incremental runs and the one-rank
communicator bit for bit.  Every test prints its figures (pytest -s).
"""
import ctypes as C
import math

import numpy as np
import pytest

import lrsim_cases as lc
from conftest import rel_l2
from spim_registration_amd import _lib
from spim_registration_amd.distributed import unique_id_bytes
from spim_registration_amd.lr_multiview import LucyRichardsonFFT, lucy_richardson_multi_view

pytestmark = pytest.mark.gpu
TOL = 1e-4
# the largest float32 ulp distance of the multiplicative rule from NumPy's double pow
# measured over the 8 x (2^20 + 77) voxels of test_update_rule_* is 0 (no voxel differs:
# DESIGN.md, "lrsim at its edges"); the bound is that plus one ulp
POW_MAX_ULP = 1


def _data(name):
    imgs, ws, ks = lc.build(name)
    return [LucyRichardsonFFT(i, w, k) for i, w, k in zip(imgs, ws, ks)]


def _run(name, mult, lam, gpu, **kw):
    stats, avg, fd = [], [], []
    psi = lucy_richardson_multi_view(_data(name), lc.CASES[name].iters, mult, lam, stats_out=stats, avg_out=avg,
                                     fft_dims_out=fd, **({"device": gpu} if "devices" not in kw else {}), **kw)
    return psi, avg[0], stats, fd


def _check(name, mult, lam, got, views_of=None):
    psi, avg, stats, fd = got
    exp, avg0, st0 = lc.oracle(name, mult, lam, views_of)
    c = lc.CASES[name]
    assert tuple(fd) == lc.padded(c.shape, c.ksizes)[::-1]
    err = rel_l2(psi, exp)
    print(f"lrsim edge {name} mult={int(mult)} lambda={lam}: psi rel-L2 {err:.2e}, avg {avg!r}")
    assert avg == pytest.approx(avg0, rel=1e-12)
    assert np.isfinite(psi).all() and (psi >= lc.MIN32).all()
    assert err < TOL, err
    np.testing.assert_allclose(np.array(stats), np.array(st0), rtol=1e-3)
    return exp


@pytest.mark.parametrize("name,mult,lam", [(n, m, l) for n, c in lc.CASES.items() for m, l in c.rules])
def test_case_matches_oracle(gpu, name, mult, lam):
    got = _run(name, mult, lam, gpu)
    exp = _check(name, mult, lam, got)
    psi, avg = got[0], got[1]
    _, ws, _ = lc.build(name)
    dead = lc.positive_count(ws) == 0
    assert (psi[dead] == lc.MIN32).all()          # no positive weight: exactly minValue
    if name == "weights":
        assert dead[lc.rows("zero")].all() and dead[lc.rows("negative")].all()
        assert np.array_equal(psi == lc.MIN32, dead)
    if name == "clamp":
        assert np.array_equal(psi == lc.MIN32, exp == lc.MIN32) and (exp == lc.MIN32).any()
    if name == "no_overlap":
        assert avg == 1.0
    if name == "delta":
        imgs, _, _ = lc.build(name)
        assert rel_l2(psi, lc.delta_closed_form(imgs, ws, avg, mult)) < TOL


@pytest.mark.parametrize("name,groups", [("odd_tail", 3), ("odd_tail", 2), ("many_rows", 2), ("many_voxels", 2)])
def test_device_groups(gpu, name, groups):
    """Two views over two groups, and over three: the third owns no view (k_lr_overlap and
    k_lr_num with nv = 0, a partial that is the merge's identity).  many_voxels: k_lr_merge's
    second trip (two of its rules, against the oracle's single merge already computed)."""
    views_of = tuple((v,) if v < 2 else () for v in range(groups))
    rules = lc.CASES[name].rules
    if name == "many_voxels":
        views_of, rules = None, rules[1:3]
    for mult, lam in rules:
        one = _run(name, mult, lam, gpu)
        many = _run(name, mult, lam, gpu, devices=[gpu] * groups)
        err = rel_l2(many[0], one[0])
        print(f"lrsim edge {name} {groups} groups mult={int(mult)}: vs one group {err:.2e}")
        assert err < 1e-6
        assert many[1] == pytest.approx(one[1], rel=1e-12)
        np.testing.assert_allclose(np.array(many[2]), np.array(one[2]), rtol=1e-6)
        _check(name, mult, lam, many, views_of)


class _Session:
    """A case driven through the C API (lucy_richardson_multi_view runs once and destroys)."""

    def __init__(self, name, gpu):
        self.lib = _lib.load()
        self.shape = lc.CASES[name].shape
        nz, ny, nx = self.shape
        self.h = C.c_void_p()
        _lib.check(self.lib.lrsim_create((C.c_int64 * 3)(nx, ny, nz), gpu, 1, 0, None, C.byref(self.h)))
        try:
            for img, w, k in zip(*lc.build(name)):
                kd = np.array(k.shape[::-1], np.int32)
                _lib.check(self.lib.lrsim_add_view(self.h, img.ctypes.data, w.ctypes.data, k.ctypes.data,
                                                   kd.ctypes.data_as(_lib._pi)))
            _lib.check(self.lib.lrsim_init(self.h, None))
        except Exception:
            self.close()
            raise

    def run(self, iters, mult, lam):
        st = np.zeros(2 * iters, np.float64)
        _lib.check(self.lib.lrsim_run(self.h, iters, int(mult), float(lam), st.ctypes.data_as(_lib._pd)))
        return st

    def psi(self):
        out = np.empty(self.shape, np.float32)
        _lib.check(self.lib.lrsim_get_psi(self.h, out.ctypes.data))
        return out

    def close(self):
        self.lib.lrsim_destroy(self.h)


@pytest.mark.parametrize("mult,lam", lc.CASES["odd_dims"].rules)
def test_incremental_runs_bit_identical(gpu, mult, lam):
    """lrsim_run(2) then lrsim_run(1) on one session == one lrsim_run(3), bit for bit."""
    out = []
    for parts in ((3,), (2, 1)):
        s = _Session("odd_dims", gpu)
        try:
            st = np.concatenate([s.run(k, mult, lam) for k in parts])
            out.append((s.psi(), st))
        finally:
            s.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1], out[1][1]) and out[0][1].size == 6
    assert lc.CASES["odd_dims"].iters == 3
    assert rel_l2(out[1][0], lc.oracle("odd_dims", mult, lam)[0]) < TOL


@pytest.mark.parametrize("name", ["odd_tail", "weights"])
def test_one_rank_communicator_bit_identical(gpu, name):
    """The all-reduces (sum / product of a double per voxel, on negative, zero and
    identity partials) and the all-gathered agreement on the data path change no bit."""
    for mult, lam in lc.CASES["odd_tail"].rules:
        a = _run(name, mult, lam, gpu)
        b = _run(name, mult, lam, gpu, nranks=1, rank=0, comm_id=unique_id_bytes())
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3]


# ------------------------------------------------------------------ the rule, voxel by voxel
def _update_rule(psi, value, num, mult, lam):
    import torch
    d = [torch.from_numpy(np.array(a)).cuda() for a in (psi, value, num)]
    out = torch.empty(psi.size, dtype=torch.float32, device="cuda")
    st = np.zeros(2, np.float64)
    _lib.check(_lib.load().lrsim_update_rule(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), psi.size, int(mult),
                                             float(lam), out.data_ptr(), st.ctypes.data_as(_lib._pd)))
    return out.cpu().numpy(), float(st[0]), float(st[1])


def _ordered(a):
    """float32 -> integers whose differences count ulps (finite values)."""
    i = a.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _check_stats(psi, got, s, mx):
    """sum |change| against math.fsum (1e-12), max |change| bit for bit; infinite alike."""
    ch = np.abs((psi - got).astype(np.float32))
    want_s, want_mx = math.fsum(ch.astype(np.float64).tolist()), float(ch.max())
    if math.isfinite(want_s):
        assert s == pytest.approx(want_s, rel=1e-12)
    else:
        assert s == want_s
    assert mx == want_mx


@pytest.mark.parametrize("lam", lc.RULE_LAMBDAS)
@pytest.mark.parametrize("specials", [True, False])
def test_update_rule_additive_bit_exact(gpu, lam, specials):
    """k_lr_update (additive; Tikhonov for lambda > 0) against apply_value + tikhonov +
    finish of the oracle, bit for bit: IEEE double * / + sqrt, rounded once to float.
    2^20 + 77 voxels: a ragged tail on a second trip, 4096 block partials."""
    psi, value, num = lc.rule_inputs(specials)
    got, s, mx = _update_rule(psi, value, num, False, lam)
    want, want_s, want_mx = lc.rule_oracle(psi, value, num, False, lam)
    assert not np.isnan(got).any() and not np.isnan(want).any()      # NaN -> minValue on both sides
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    _check_stats(psi, got, s, mx)
    assert mx == want_mx and (s == want_s or s == pytest.approx(want_s, rel=1e-12))
    if not specials:
        assert math.isfinite(s) and math.isfinite(mx)


@pytest.mark.parametrize("lam", lc.RULE_LAMBDAS)
@pytest.mark.parametrize("specials", [True, False])
def test_update_rule_multiplicative(gpu, lam, specials):
    """k_lr_update (multiplicative) against NumPy's double pow: the same voxels clamped to
    minValue (NaN included) and infinite, the others within POW_MAX_ULP float32 ulps
    (neither pow is correctly rounded)."""
    psi, value, num = lc.rule_inputs(specials)
    got, s, mx = _update_rule(psi, value, num, True, lam)
    want, _, _ = lc.rule_oracle(psi, value, num, True, lam)
    assert not np.isnan(got).any()
    assert np.array_equal(got == lc.MIN32, want == lc.MIN32)
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    ulp = np.abs(_ordered(got[fin]) - _ordered(want[fin]))
    print(f"lrsim rule mult lambda={lam} specials={specials}: max ulp {int(ulp.max())}, "
          f"share differing {float((ulp > 0).mean()):.2e}, clamped {int((want == lc.MIN32).sum())}")
    assert ulp.max() <= POW_MAX_ULP
    _check_stats(psi, got, s, mx)
