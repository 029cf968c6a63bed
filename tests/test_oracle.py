"""CPU tests of the oracle (oracle/vro.c) against its unit-level pins.

The reference ships no tests, fixtures or golden vectors.
Whole images are pinned elsewhere: tests/test_reference_fixtures.py compares
the oracle bit for bit with images the reference's own kernel source rendered
when compiled for the host (oracle/ref/, DESIGN.md "Oracle").  Here the
oracle's parts are pinned by:
  * RNG known answers produced by rocThrust itself (the third-party
    dependency the reference kernel uses), tests/golden/rng_kat.json;
  * the values SURVEY.md 8c recorded from its probe run of the reference
    kernel (centre pixel exact to the printed digits; the image mean, a
    chaotic statistic, to 5e-4 relative);
  * analytic known answers for the intersection and index primitives.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import pyoracle as po

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_f = ctypes.POINTER(ctypes.c_float)


def f4(*v):
    a = (ctypes.c_float * 4)(*([float(x) for x in v] + [0.0] * (4 - len(v))))
    return a


def default_cam():
    from vrenderer_pathtracer_amd.scenes import default_camera
    return default_camera()


def test_rng_engine_matches_rocthrust(oracle):
    kat = json.load(open(os.path.join(GOLDEN, "rng_kat.json")))
    L = oracle.lib()
    for e in kat["engine"]:
        out = np.zeros(len(e["u_bits"]), np.float32)
        L.vro_rng_uniforms(e["seed"] & 0xFFFFFFFF, out.size, out.ctypes.data_as(_f))
        assert out.view(np.uint32).tolist() == e["u_bits"], e["seed"]


def test_rng_pixel_seeds_match_rocthrust(oracle):
    """hash() seed chaining across the two samples of a pixel (PathTracer.cu:574-580,817-818)."""
    kat = json.load(open(os.path.join(GOLDEN, "rng_kat.json")))
    L = oracle.lib()
    for px in kat["pixel"]:
        s0 = ctypes.c_uint32((px["x"] * px["frame"]) & 0xFFFFFFFF)
        s1 = ctypes.c_uint32((px["y"] * px["time"]) & 0xFFFFFFFF)
        for smp in px["samples"]:
            seed = L.vro_hash(ctypes.byref(s0), ctypes.byref(s1))
            assert seed == smp["seed"]
            out = np.zeros(3, np.float32)
            L.vro_rng_uniforms(seed, 3, out.ctypes.data_as(_f))
            assert out.view(np.uint32).tolist() == smp["u_bits"]


def test_survey_rng_kats(oracle):
    """SURVEY.md 8a R10 known answers."""
    L = oracle.lib()
    s0, s1 = ctypes.c_uint32(100 * 1), ctypes.c_uint32(50 * 12345)
    assert L.vro_hash(ctypes.byref(s0), ctypes.byref(s1)) == 0x88266ba4
    out = np.zeros(3, np.float32)
    L.vro_rng_uniforms(0x88266ba4, 3, out.ctypes.data_as(_f))
    np.testing.assert_allclose(out, [0.535258412, 0.459824145, 0.171328396], rtol=1e-8)
    assert L.vro_hash(ctypes.byref(s0), ctypes.byref(s1)) == 0xcfc8cb90


@pytest.mark.parametrize("libm", [po.LIBM_GLIBC, po.LIBM_PORTABLE])
def test_survey_probe_values(oracle, libm):
    """SURVEY.md 8c sanity values of the reference kernel run as a host program:
    Cornell + example sphere, 512x512, 4 frames, _time=12345, default camera."""
    sc = dict(camera=default_cam(), width=512, height=512, cornell=True, example_sphere=True, time=12345)
    acc, _, _, _ = po.render(sc, frames=4, libm=libm)
    centre = acc[256, 256, :3] / 4
    np.testing.assert_allclose(centre, [0.06276, 0.06049, 0.02766], atol=6e-6)
    mean = float((acc[..., :3] / 4).sum(-1).mean())
    assert abs(mean - 0.864683) / 0.864683 < 5e-4, mean


def test_survey_probe_without_example_sphere(oracle):
    sc = dict(camera=default_cam(), width=512, height=512, cornell=True, example_sphere=False, time=12345)
    acc, _, _, _ = po.render(sc, frames=4)
    mean = float((acc[..., :3] / 4).sum(-1).mean())
    assert abs(mean - 0.887841) / 0.887841 < 5e-4, mean


def _ulp(x):
    x = np.abs(np.asarray(x, np.float32))
    return np.where(x > 0, np.spacing(x), np.float32(1.4e-45)).astype(np.float64)


@pytest.mark.parametrize("name,ref,lo,hi,tol", [
    ("vro_p_sinf", np.sin, 0.0, 2 * math.pi, 0.501),
    ("vro_p_cosf", np.cos, 0.0, 2 * math.pi, 0.501),
    ("vro_p_sinf", np.sin, -30.0, 30.0, 0.501),
    ("vro_p_acosf", np.arccos, -1.0, 1.0, 1.0),
])
def test_portable_libm_unary_accuracy(oracle, name, ref, lo, hi, tol):
    L = oracle.lib()
    f = getattr(L, name)
    x = np.random.default_rng(0).uniform(lo, hi, 20000).astype(np.float32)
    got = np.array([f(float(v)) for v in x], np.float64)
    exact = ref(x.astype(np.float64))
    err = np.abs(got - exact) / _ulp(exact)
    assert err.max() <= tol, err.max()


@pytest.mark.parametrize("case", ["atan2", "pow_fresnel", "pow_brdf", "pow_gamma"])
def test_portable_libm_binary_accuracy(oracle, case):
    L = oracle.lib()
    rng = np.random.default_rng(1)
    n = 20000
    if case == "atan2":
        y, x = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
        f, ref, tol = L.vro_p_atan2f, np.arctan2, 1.5
    elif case == "pow_fresnel":
        y, x = rng.uniform(0, 2, n), rng.uniform(0.1, 8, n)   # (base, exponent)
        f, ref, tol = L.vro_p_powf, np.power, 0.501
    elif case == "pow_brdf":
        y, x = rng.uniform(0.5, 1.5, n), np.full(n, -1.5)
        f, ref, tol = L.vro_p_powf, np.power, 0.501
    else:
        y, x = rng.uniform(0, 1, n), np.full(n, 1 / 2.2)
        f, ref, tol = L.vro_p_powf, np.power, 0.501
    a = y.astype(np.float32)
    b = x.astype(np.float32)
    got = np.array([f(float(u), float(v)) for u, v in zip(a, b)], np.float64)
    exact = ref(a.astype(np.float64), b.astype(np.float64))
    err = np.abs(got - exact) / _ulp(exact)
    assert err.max() <= tol, err.max()


def test_portable_pow_special_cases(oracle):
    p = oracle.lib().vro_p_powf
    assert p(-2.0, 3.0) == -8.0
    assert p(0.0, -1.5) == math.inf
    assert math.isnan(p(-0.5, 0.3))
    assert p(5.0, 0.0) == 1.0 and p(1.0, math.nan) == 1.0
    assert p(0.0, 2.0) == 0.0


def test_intersect_triangle_known_answers(oracle):
    L = oracle.lib()
    out = (ctypes.c_float * 4)()
    v0, v1, v2 = f4(-1, -1, 0), f4(1, -1, 0), f4(0, 1, 0)
    L.vro_intersect_triangle(v0, v1, v2, f4(0, 0, 5), f4(0, 0, -1), out)
    assert list(out)[:3] == [5.0, 0.25, 0.5]
    L.vro_intersect_triangle(v0, v1, v2, f4(3, 0, 5), f4(0, 0, -1), out)      # misses (u > 1)
    assert list(out) == [0, 0, 0, 0]
    L.vro_intersect_triangle(v0, v1, v2, f4(0, 0, 5), f4(1, 0, 0), out)       # parallel: |det| < eps
    assert list(out) == [0, 0, 0, 0]
    L.vro_intersect_triangle(v0, v1, v2, f4(0, 0, 5), f4(0, 0, 1), out)       # behind: t < 0
    assert list(out) == [0, 0, 0, 0]
    L.vro_intersect_triangle(v0, v2, v1, f4(0, 0, -5), f4(0, 0, 1), out)      # no back-face culling
    assert out[0] == 5.0


def test_sphere_intersect_known_answers(oracle):
    L = oracle.lib()
    o, d = f4(0, 0, 150), f4(0, 0, -1)
    assert L.vro_sphere_intersect(8, o, d) == 140.0            # example sphere r=10 at origin
    assert L.vro_sphere_intersect(3, o, d) == 250.0            # back wall at z = -100
    assert L.vro_sphere_intersect(7, f4(25, 0, 15), d) == 3.5  # inside the grey sphere: far root
    assert L.vro_sphere_intersect(6, f4(0, 0, 15), f4(0, 1, 0)) == 0.0


def test_span_integer_semantics(oracle):
    """Kepler spans on int bit patterns (MathHelpers.cuh:454-552) equal the
    float definitions wherever the visit decision depends on them."""
    L = oracle.lib()
    rng = np.random.default_rng(2)
    be = (ctypes.c_float * 2)()
    for _ in range(3000):
        s = rng.uniform(-50, 50, 6).astype(np.float32)
        L.vro_span((ctypes.c_float * 6)(*s.tolist()), be)
        fb = max(min(s[0], s[1]), min(s[2], s[3]), min(s[4], s[5]), 0.0)
        fe = min(max(s[0], s[1]), max(s[2], s[3]), max(s[4], s[5]), 1e20)
        assert be[0] == np.float32(fb)
        assert (be[1] >= be[0]) == (np.float32(fe) >= np.float32(fb))


def _brdf_index_py(theta_half, theta_diff, phi_diff):
    """MERL index maps, PathTracer.cu:473-506 (float32 pi, double literals)."""
    PI = float(np.float32(3.14159265359))
    if phi_diff < 0.0:
        phi_diff = float(np.float32(phi_diff + math.pi))
    pdi = min(max(int(phi_diff * (1.0 / PI * 180)), 0), 179)
    thi = 0 if theta_half <= 0.0 else min(max(int(np.float32(np.sqrt(np.float32(theta_half * (2.0 / PI)))) * np.float32(90)), 0), 89)
    tdi = min(max(int(theta_diff * (2.0 / PI * 90)), 0), 89)
    return pdi + tdi * 180 + thi * 180 * 90


def test_brdf_index_mirror_and_grazing(oracle):
    L = oracle.lib()
    n, t = f4(0, 1, 0), f4(1, 0, 0)
    # reflected == mirror of incoming: H == n, theta_h = 0, theta_d = angle(H, refl)
    s = math.sqrt(0.5)
    idx = L.vro_brdf_index(f4(s, s, 0), f4(-s, -s, 0), n, t, po.LIBM_GLIBC)
    assert idx == L.vro_brdf_index(f4(s, s, 0), f4(-s, -s, 0), n, t, po.LIBM_PORTABLE)
    assert 0 <= idx < 1458000
    idx2 = L.vro_brdf_index(f4(0, 1, 0), f4(0, -1, 0), n, t, po.LIBM_GLIBC)   # theta_h = theta_d = 0
    assert idx2 == _brdf_index_py(0.0, 0.0, 0.0)


def test_glibc_and_portable_oracles_agree(oracle):
    from vrenderer_pathtracer_amd import scenes
    for cfg, w, h in [("C1", 96, 64), ("C3", 96, 64)]:
        sc = scenes.make_scene(cfg, w, h)
        a, _, _, _ = po.render(sc, frames=2, libm=po.LIBM_GLIBC)
        b, _, _, _ = po.render(sc, frames=2, libm=po.LIBM_PORTABLE)
        d = a[..., :3] / 2 - b[..., :3] / 2
        assert float(np.sqrt((d ** 2).mean())) < 1e-3
        assert (np.abs(d).max(-1) <= 1e-3).mean() > 0.999


def test_oracle_row_ranges_compose(oracle):
    """Rendering row ranges separately equals one full render (bounded CPU samples)."""
    from vrenderer_pathtracer_amd import scenes
    sc = scenes.make_scene("C2", 64, 48)
    full, _, _, _ = po.render(sc, frames=1)
    part = np.zeros_like(full)
    for r0 in (0, 16, 32):
        po.render(sc, frames=1, rows=(r0, r0 + 16), accum=part)
    assert np.array_equal(full.view(np.uint32), part.view(np.uint32))


def test_oracle_counts_plausible(oracle):
    from vrenderer_pathtracer_amd import scenes
    sc = scenes.make_scene("C2", 64, 48)
    _, _, _, c = po.render(sc, frames=1, count=True)
    assert c["paths"] == 64 * 48 * 2
    assert 3.9 <= c["rays"] / c["paths"] <= 4.0          # Cornell paths almost always bounce 4 times
    assert c["max_stack"] <= 30
