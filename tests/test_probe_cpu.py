"""The probe query's yardstick on the CPU (tests/probe_driver.c,
tests/probe_cases.py; vrhip_probe_sh, vrhip_sh_irradiance): the driver against
closed forms and a float64 projection, the mutants it must tell apart, the
case set's oracle records, the direction sets and the refusals that need no
device.

The bound.  A coefficient is the fixed-order fp32 sum of the terms
t_k = (w_k * Y_j(d_k)) * L_k.  A term carries at most four roundings beyond
its float64 value on the same unit vector (the basis polynomial's last
product and the two products of the term, and one for the operations inside
the polynomial relative to its size; the normalisation is done in float64
from the same fp32 inputs on both sides only up to its own two roundings,
which the fourth covers for these well-conditioned sets); the tree adds six
roundings to every slot's path and the block partials n_blocks more.  Each
rounding is at most 2^-24 of a partial sum no larger than sum |t_k|, so
    |driver - float64| <= (6 + n_blocks + 4) * 2^-24 * sum |t_k|.
Against a closed form the set's own quadrature error is added, computed in
float64 from the same directions and never from the code under test.
"""
import ctypes
import math

import numpy as np
import pytest

import probe_cases as pc
import radiance_cases as rc
from vrenderer_pathtracer_amd import scenes

EPS, A_BAND = pc.EPS, pc.A_BAND
basis64, unit64, project64, bound_of = pc.basis64, pc.unit64, pc.project64, pc.bound_of


def coeffs(words):
    return np.ascontiguousarray(words).view(np.float32)[:, :27].reshape(-1, 9, 3).astype(np.float64)


def run(rec, dirs, weights=None, valid=None, mutant=0):
    rec = np.asarray(rec, np.float32)
    v = np.ones(rec.shape[:2], np.uint8) if valid is None else valid
    return pc.project(rec, dirs, weights, v, mutant)


# ---- 1. closed forms ------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [True, False], ids=["compact", "fibonacci"])
def test_uniform_records(compact):
    """One colour L from every direction: coefficient 0 is 2 sqrt(pi) L, the
    others vanish, and the irradiance is pi L at any unit normal."""
    k = 1024
    d, w = scenes.probe_directions(k, compact)
    L = np.array([0.75, 1.5, 0.03125], np.float32)
    rec = np.zeros((1, k, 4), np.float32)
    rec[:, :, :3] = L
    for weights in (None, w):
        words = run(rec, d, weights)
        assert words[0, 27] == k
        exact, abs_sum = project64(rec, d, weights)
        want = np.zeros((9, 3))
        want[0] = 2.0 * math.sqrt(math.pi) * L.astype(np.float64)
        tol = bound_of(abs_sum[0], k) + np.abs(exact[0] - want)           # rounding + the set's quadrature error
        got = coeffs(words)[0]
        assert (np.abs(got - want) <= tol).all(), (np.abs(got - want) / tol).max()
        assert (tol[0] < 1e-5 * want[0]).all() and (tol[1:] < 1e-3).all()     # the bound is a bound, not a licence
        # irradiance: the driver's evaluation against pi L
        rng = np.random.default_rng(3)
        n = unit64(rng.normal(size=(64, 3))).astype(np.float32)
        E = pc.irradiance(words, n, np.zeros(len(n), np.uint32))
        etol = pc.irradiance_bound(n, got, tol, L)
        assert (np.abs(E[:, :3] - math.pi * L.astype(np.float64)) <= etol).all()
        assert not E[:, 3].any()


def test_clamped_cosine_records():
    """L = max(0, d . a): band l of the projection is A_l * Y_lm(a), i.e.
    (sqrt(pi) / 2, sqrt(pi / 3) * a, ...)."""
    k = 1024
    d, w = scenes.probe_directions(k)
    rng = np.random.default_rng(11)
    axes = unit64(rng.normal(size=(5, 3)))
    u = unit64(d)
    rec = np.zeros((len(axes), k, 4), np.float32)
    rec[:, :, :3] = np.maximum(0.0, axes @ u.T)[:, :, None]
    words = run(rec, d, w)
    exact, abs_sum = project64(rec, d, w)
    want = (A_BAND[None, :] * basis64(axes))[:, :, None].repeat(3, -1)
    assert abs(want[0, 0, 0] - math.sqrt(math.pi) / 2) < 1e-12
    assert np.allclose(want[:, [3, 1, 2], 0], math.sqrt(math.pi / 3.0) * axes, atol=1e-12)
    tol = bound_of(abs_sum, k) + np.abs(exact - want)
    got = coeffs(words)
    assert (np.abs(got - want) <= tol).all(), (np.abs(got - want) / tol).max()
    assert (tol < 0.02).all()                              # 1,024 directions resolve the lobe's kink to a percent


# ---- 2. float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dirs", [1, 63, 64, 65, 130, 192, 1000])
def test_driver_against_float64(n_dirs):
    rng = np.random.default_rng(100 + n_dirs)
    d = (unit64(rng.normal(size=(n_dirs, 3))) * rng.uniform(0.1, 10.0, (n_dirs, 1))).astype(np.float32)
    w = rng.uniform(0.0, 0.3, n_dirs).astype(np.float32)
    rec = rng.uniform(0.0, 4.0, (9, n_dirs, 4)).astype(np.float32)
    for weights in (None, w):
        words = run(rec, d, weights)
        exact, abs_sum = project64(rec, d, weights)
        assert (np.abs(coeffs(words) - exact) <= bound_of(abs_sum, n_dirs)).all()
        assert (words[:, 27] == n_dirs).all()


def test_invalid_rays_contribute_plus_zero():
    rng = np.random.default_rng(5)
    k = 130
    d, w = scenes.probe_directions(k)
    w = w.copy()
    rec = rng.uniform(0.0, 2.0, (3, k, 4)).astype(np.float32)
    valid = np.ones((3, k), np.uint8)
    valid[0, [0, 31, 63, 64]] = 0
    valid[1, :] = 0
    w[31] = np.nan                                         # on an invalid ray of probe 0, a valid one of probe 2
    words = run(rec, d, w, valid)
    assert list(words[:, 27]) == [k - 4, 0, k]
    assert np.isfinite(coeffs(words)[0]).all()
    assert not words[1, :27].any()                          # every coefficient +0, bit for bit
    assert np.isnan(coeffs(words)[2]).all()
    rec0 = rec.copy()
    rec0[0, [0, 31, 63, 64]] = 0
    w0 = w.copy()
    w0[31] = 0
    assert (run(rec0[:1], d, w0)[0, :27] == words[0, :27]).all()


# ---- 3. the case set and its mutants ---------------------------------------------------------------
def case_outputs(mutant):
    """Every output word of the CPU case set under `mutant`: the oracle's
    records of one combination at every direction count, a case with invalid
    rays under a NaN weight, and the expanded seeds of the probe set."""
    name = "cornell+mesh"
    out = [pc.oracle_records(name, n, 2, mutant) for n in pc.N_DIRS]
    pts, d, w, ps, ds = pc.probe_set()
    # invalid rays: a NaN point (probe 1), a zero direction (slot 5) with a NaN weight
    p2, d2, w2 = pts[:4].copy(), d[:65].copy(), w[:65].copy()
    p2[1, 0] = np.nan
    d2[5] = 0
    w2[5] = np.nan
    rec = rc.record_of(pc.reference(name)[:4, :65].reshape(-1, rc.K_MAX, 4), 2).reshape(4, 65, 4)
    out.append(pc.project(rec, d2, w2, pc.valid_rays(p2, d2), mutant))
    out.append(pc.expand(pts, d, ps, ds, mutant)[2])
    return out


def test_case_set_meets_the_oracle_condition(oracle):
    """At most 1 % of the probes have a non-finite oracle coefficient, in every
    combination and at every sample count of test_gpu_probe.py."""
    for name in rc.COMBO_NAMES:
        for k in rc.SAMPLES:
            words = pc.oracle_records(name, pc.K_DIRS, k)
            pc.finite_probes(words)
            assert (words[:, 27] == pc.K_DIRS).all()
        assert np.any(coeffs(words) != 0)


@pytest.mark.parametrize("mutant", sorted(pc.MUTANTS))
def test_mutants_change_the_case_set(oracle, mutant):
    base, mut = case_outputs(0), case_outputs(mutant)
    changed = sum(int((a != b).sum()) for a, b in zip(base, mut))
    total = sum(a.size for a in base)
    print(f"mutant {mutant} ({pc.MUTANTS[mutant]}): {changed} of {total} words differ")
    assert changed > 0, pc.MUTANTS[mutant]
    if mutant == 5:                                         # other seeds are other paths: the records move too
        pts, d, _, ps, ds = pc.probe_set()
        import flag_lattice as fl
        sc = fl.scene_of(rc.combo_of("cornell+mesh"))
        words = []
        for m in (0, 5):
            o, dd, s = pc.expand(pts[:4], d[:65], ps[:4], ds[:65], m)
            rec = rc.oracle_radiance(sc, o, dd, s, 2).reshape(4, 65, 4)
            words.append(pc.project(rec, d[:65], None, pc.valid_rays(pts[:4], d[:65])))
        assert (words[0] == pc.oracle_records("cornell+mesh", 65, 2)[:4]).all()
        assert (words[0] != words[1]).any()


# ---- 4. direction sets --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 64, 192, 256, 1024])
def test_probe_directions(k):
    d, w = scenes.probe_directions(k, compact=False)
    c, wc = scenes.probe_directions(k, compact=True)
    assert d.dtype == c.dtype == w.dtype == np.float32 and d.shape == c.shape == (k, 3) and w.shape == (k,)
    assert (w == wc).all() and (w == np.float32(12.566370614) / np.float32(k)).all()
    assert np.allclose((d.astype(np.float64) ** 2).sum(-1), 1.0, atol=1e-6)
    # the same set, reordered
    assert (np.sort(d.view([("", np.float32)] * 3).ravel()) == np.sort(c.view([("", np.float32)] * 3).ravel())).all()
    if k in (256, 1024):
        # a block of the compact order is a cap, a Fibonacci block a band round the sphere: the mean of a cap of
        # 64 / k of the sphere has length 1 - 64 / k, the mean of a band lies near the axis
        def spread(a):
            return np.linalg.norm(a.reshape(-1, 64, 3).astype(np.float64).mean(1), axis=-1).mean()
        assert spread(c) > 0.9 * (1.0 - 64.0 / k) and spread(d) < 0.55


# ---- 5. refusals that need no device -------------------------------------------------------------------
def test_null_context_is_invalid(native):
    assert native.vrhip_probe_sh(None, None, None, None, None, None, 0, 1, 1, None) == -1
    assert native.vrhip_probe_sh(None, None, None, None, None, None, 4, 64, 2, None) == -1
    assert native.vrhip_sh_irradiance(None, None, 0, None, None, 0, None) == -1
    assert b"null ctx" in native.vrhip_last_error()
    assert isinstance(native.vrhip_probe_sh.restype, type(ctypes.c_int)) or native.vrhip_probe_sh.restype is ctypes.c_int
