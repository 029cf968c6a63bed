"""Probes, directions and the yardstick shared by the probe-query tests
(test_probe_cpu.py, test_gpu_probe.py; vrhip_probe_sh, vrhip_sh_irradiance).

The yardstick is tests/probe_driver.c: the projection and the irradiance
evaluation of include/vrhip.h restated in plain C and compiled with the
oracle's CFLAGS (-ffp-contract=off).  Its inputs are per-ray radiance records,
the directions, the weights and a validity flag per ray, so it is a yardstick
whether the records come from the oracle (radiance_cases.oracle_radiance on the
expanded rays) or from traceRadiance.  Its `mutant` argument selects one of
seven deliberately wrong projections; test_probe_cpu.py shows that each of
them changes the output on the case set.

Probe points lie at scene scale, inside the Cornell box and around the mesh
bounds: they are origins of radiance_cases.ray_set("B").  A record word that is
not finite is compared as "NaN in both"; PROBES is chosen so that the oracle
alone gives at most MAX_DROPPED of the probes such a word (asserted on the CPU).
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
import subprocess

import numpy as np

import flag_lattice as fl
import pyoracle as po
import radiance_cases as rc
import surface_cases as sf

_HERE = os.path.dirname(os.path.abspath(__file__))
_DRIVER_SRC = os.path.join(_HERE, "probe_driver.c")
_DRIVER_LIB = os.path.join(_HERE, "libprobe_driver.so")

BLOCK, WORDS = 64, 28                # VRHIP_PROBE_BLOCK, VRHIP_PROBE_WORDS
MUTANTS = {1: "sequential instead of tree order", 2: "a block of 32", 3: "Y6 contracted into an fma",
           4: "(Y * L) * w", 5: "seeds combined with +", 6: "an invalid ray contributes w * Y * 0",
           7: "the tail padded with the last term"}
N_PROBES = 70                        # more than one wave of probes, no multiple of anything
N_DIRS = (1, 63, 64, 65, 130, 192)   # a lone lane, a block one short, an exact block, a one-lane tail, two and three blocks
K_DIRS = max(N_DIRS)
MAX_DROPPED = 0.01                   # probes with a non-finite oracle coefficient


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the driver -------------------------------------------------------------------
def build_driver() -> str:
    srcs = [_DRIVER_SRC, os.path.join(sf._ORACLE, "Makefile")]
    if not os.path.exists(_DRIVER_LIB) or os.path.getmtime(_DRIVER_LIB) < max(os.path.getmtime(s) for s in srcs):
        tmp = f"{_DRIVER_LIB}.tmp{os.getpid()}"
        cmd = [os.environ.get("CC", "gcc")] + sf.oracle_cflags() + ["-shared", "-o", tmp, _DRIVER_SRC, "-lm"]
        subprocess.run(cmd, check=True)
        os.replace(tmp, _DRIVER_LIB)
    return _DRIVER_LIB


@functools.lru_cache(maxsize=None)
def driver():
    L = ctypes.CDLL(build_driver())
    vp, u = ctypes.c_void_p, ctypes.c_uint32
    L.probe_expand_seeds.restype = None
    L.probe_expand_seeds.argtypes = [vp, vp, u, u, u, vp]
    L.probe_project.restype = ctypes.c_int
    L.probe_project.argtypes = [vp, vp, vp, vp, u, u, u, vp]
    L.probe_irradiance.restype = ctypes.c_int
    L.probe_irradiance.argtypes = [vp, u, vp, vp, u, vp]
    return L


def valid_rays(points, dirs) -> np.ndarray:
    """[P, K] bool: the radiance query's rule on ray (i, k) -- six finite
    floats and an fp32 dx*dx + dy*dy + dz*dz that is finite and above 0."""
    p, d = np.asarray(points, np.float32), np.asarray(dirs, np.float32)
    with np.errstate(all="ignore"):
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        dk = np.isfinite(d).all(-1) & (dd > 0) & np.isfinite(dd)
    assert dd.dtype == np.float32
    return np.isfinite(p).all(-1)[:, None] & dk[None, :]


def expand(points, dirs, probe_seeds, dir_seeds, mutant=0):
    """The P * K rays of a probe call as traceRadiance takes them, probe-major:
    (origins [PK,3], dirs [PK,3], seeds [PK,2] by the XOR rule)."""
    p, d = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(dirs, np.float32)
    ps, ds = np.ascontiguousarray(probe_seeds, np.uint32), np.ascontiguousarray(dir_seeds, np.uint32)
    P, K = len(p), len(d)
    seeds = np.empty((P * K, 2), np.uint32)
    driver().probe_expand_seeds(ps.ctypes.data, ds.ctypes.data, P, K, mutant, seeds.ctypes.data)
    return np.repeat(p, K, 0), np.tile(d, (P, 1)), seeds


def project(rec, dirs, weights, valid, mutant=0) -> np.ndarray:
    """[P, 28] uint32: the records of vrhip_probe_sh from the radiance records
    rec [P, K, 4] of its rays."""
    rec = np.ascontiguousarray(rec, np.float32)
    P, K = rec.shape[:2]
    d = np.ascontiguousarray(dirs, np.float32)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    v = np.ascontiguousarray(valid, np.uint8)
    assert rec.shape == (P, K, 4) and d.shape == (K, 3) and v.shape == (P, K) and (w is None or w.shape == (K,))
    out = np.zeros((P, WORDS), np.uint32)
    err = driver().probe_project(rec.ctypes.data, d.ctypes.data, None if w is None else w.ctypes.data, v.ctypes.data,
                                 P, K, mutant, out.ctypes.data)
    assert err == 0, err
    return out


def irradiance(sh, normals, index=None) -> np.ndarray:
    """[n, 4] float32: vrhip_sh_irradiance by the driver; sh [m, 28] as uint32 or float32 words."""
    s = np.ascontiguousarray(sh).view(np.float32).reshape(-1, WORDS)
    nr = np.ascontiguousarray(normals, np.float32)
    ix = None if index is None else np.ascontiguousarray(index, np.uint32)
    out = np.zeros((len(nr), 4), np.float32)
    err = driver().probe_irradiance(s.ctypes.data, len(s), None if ix is None else ix.ctypes.data, nr.ctypes.data,
                                    len(nr), out.ctypes.data)
    assert err == 0, err
    return out


def same_words(got, want) -> np.ndarray:
    """Per record: all 28 words equal as uint32; a coefficient may instead be NaN in both."""
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    gf, wf = g.view(np.float32), w.view(np.float32)
    nan = np.isnan(gf) & np.isnan(wf)
    nan[..., WORDS - 1:] = False                          # the count is an integer
    return ((g == w) | nan).all(-1)


# ---- the case set -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe_set():
    """(points [N_PROBES,3], dirs [K_DIRS,3], weights [K_DIRS], probe_seeds
    [N_PROBES,2], dir_seeds [K_DIRS,2]), never written.  The points are origins
    of ray set B; the directions a compact Fibonacci set scaled by lengths in
    [0.5, 2] (the library normalises), the first n of which serve every n_dirs;
    the weights positive and unequal."""
    from vrenderer_pathtracer_amd import scenes
    rng = np.random.default_rng(20250117)
    pts = rc.ray_set("B")[0][:N_PROBES]
    d, _ = scenes.probe_directions(K_DIRS, compact=True)
    d = (d.astype(np.float64) * rng.uniform(0.5, 2.0, (K_DIRS, 1))).astype(np.float32)
    w = rng.uniform(0.01, 0.2, K_DIRS).astype(np.float32)
    ps = rng.integers(0, 2**32, (N_PROBES, 2), dtype=np.uint64).astype(np.uint32)
    ds = rng.integers(0, 2**32, (K_DIRS, 2), dtype=np.uint64).astype(np.uint32)
    out = tuple(np.ascontiguousarray(a) for a in (pts, d, w, ps, ds))
    assert not (np.signbit(out[1]) & (out[1] == 0)).any(), "the yardstick's camera sum can turn a -0 into +0"
    for a in out:
        a.setflags(write=False)
    return out


def weights_for(n_dirs):
    """Explicit weights for the even direction counts, the default for the odd ones."""
    return probe_set()[2][:n_dirs] if n_dirs % 2 == 0 else None


@functools.lru_cache(maxsize=None)
def reference(name, mesh="shallow"):
    """paths [N_PROBES, K_DIRS, K_MAX, 4] of combination `name` on the rays of
    probe_set(): computed once, shared by every test that needs it, never
    written.  Ray (i, k) does not depend on n_dirs, so a call with n
    directions takes [:, :n]."""
    po.build()
    pts, d, _, ps, ds = probe_set()
    o, dd, s = expand(pts, d, ps, ds)
    paths = rc.oracle_paths(fl.scene_of(rc.combo_of(name), mesh), o, dd, s, rc.K_MAX)
    paths = paths.reshape(N_PROBES, K_DIRS, rc.K_MAX, 4)
    paths.setflags(write=False)
    return paths


def oracle_records(name, n_dirs, samples, mutant=0, mesh="shallow") -> np.ndarray:
    """[N_PROBES, 28] uint32: the oracle's radiance records through the driver."""
    pts, d, _, _, _ = probe_set()
    paths = reference(name, mesh)[:, :n_dirs]
    rec = rc.record_of(paths.reshape(-1, rc.K_MAX, 4), samples).reshape(N_PROBES, n_dirs, 4)
    return project(rec, d[:n_dirs], weights_for(n_dirs), valid_rays(pts, d[:n_dirs]), mutant)


def finite_probes(words) -> np.ndarray:
    """The probes whose 27 coefficients are all finite; at most MAX_DROPPED may fail."""
    ok = np.isfinite(np.ascontiguousarray(words).view(np.float32)[:, :WORDS - 1]).all(-1)
    assert (~ok).sum() <= MAX_DROPPED * len(ok), f"{(~ok).sum()} of {len(ok)} probes have a non-finite oracle coefficient"
    return ok


# ---- float64 and the derived bound (test_probe_cpu.py has the derivation) --------------------------
EPS = 2.0 ** -24
A_BAND = np.array([math.pi] + [2.0 * math.pi / 3.0] * 3 + [math.pi / 4.0] * 5)


def basis64(d):
    """Y0..Y8 in float64 on unit vectors [n,3]."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([np.full(len(d), 0.28209479177387814), 0.4886025119029199 * y, 0.4886025119029199 * z,
                     0.4886025119029199 * x, 1.0925484305920792 * x * y, 1.0925484305920792 * y * z,
                     0.31539156525252005 * (3.0 * z * z - 1.0), 1.0925484305920792 * x * z,
                     0.5462742152960396 * (x * x - y * y)], -1)


def unit64(d):
    d = np.asarray(d, np.float64)
    return d / np.sqrt((d * d).sum(-1, keepdims=True))


def project64(rec, dirs, weights):
    """(coefficients [P,9,3], sum |t| [P,9,3]) in float64 from fp32 inputs."""
    Y = basis64(unit64(dirs))
    w = np.full(len(dirs), float(np.float32(12.566370614) / np.float32(len(dirs)))) if weights is None \
        else np.asarray(weights, np.float64)
    t = (w[None, :, None, None] * Y[None, :, :, None]) * np.asarray(rec, np.float64)[:, :, None, :3]
    return t.sum(1), np.abs(t).sum(1)


def bound_of(abs_sum, n_dirs):
    return (6 + -(-n_dirs // BLOCK) + 4) * EPS * abs_sum


def irradiance_bound(normals, coeff, coeff_tol, L):
    """[n, 3]: how far the fp32 irradiance of coefficients `coeff` [9,3], each
    within coeff_tol [9,3] of uniform radiance L's, may lie from pi L at unit
    normals: the coefficients' own tolerance carried through the lobe, 16
    roundings on the nine terms of the evaluation (three products and the
    basis polynomial per term, eight sums), and the normals being unit to fp32
    only (|n|^2 - 1 is 2^-23 at most, which moves Y6 and the band-2 terms)."""
    Yn = np.abs(basis64(np.asarray(normals, np.float64)))
    lobe = A_BAND[None, :] * Yn
    carried = (lobe[:, :, None] * np.asarray(coeff_tol)[None]).sum(1)
    terms = np.abs(lobe[:, :, None] * np.asarray(coeff)[None]).sum(1)
    return carried + 16 * EPS * terms + 4 * EPS * math.pi * np.asarray(L, np.float64)
