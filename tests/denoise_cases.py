"""Inputs and the yardstick shared by the denoiser tests (test_denoise_cpu.py,
test_gpu_denoise.py; vrhip_denoise, vrhip_denoise_frame).

The yardstick is tests/denoise_driver.c: the filter's pixelwise definition
(include/vrhip.h) restated in plain C and compiled with the oracle's CFLAGS
(-ffp-contract=off), so that the kernels must give its bits.  -DMUTANT=k
builds one of five deliberately wrong filters; test_denoise_cpu.py shows that
every parity case notices the mutants it claims to cover.

Parity inputs are synthetic grids (grid): a tilted, bumpy height field split
into three regions of different base normals, with per-cell normal noise of
widely varying amplitude (so that dn lies near 1 as well as far below it: the
normal weight is tested at m = 0 and at m = 7, where dn^128 is inside
(0.01, 0.99) only for dn in (0.965, 0.9999)), albedos that include 0, 0x1p-8f
and its next float up, and about one invalid cell in eight (kind 0, 5 and
0xFFFFFFFF).  The condition every case must meet (check_condition): each of
wn, wp and wc lies strictly inside (0.01, 0.99) on at least 5 % of the
evaluated taps; a case that fails it tests nothing of that term.  The one
exception is the 1 x 1 grid, whose only tap is the centre, where wp and wc are
1 by definition: it stays a parity case (the smallest grid) and is exempt.
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np

import surface_cases as sf

_HERE = os.path.dirname(os.path.abspath(__file__))
_DRIVER_SRC = os.path.join(_HERE, "denoise_driver.c")

DEMODULATE = 1                                          # VRHIP_DENOISE_DEMODULATE
MUTANTS = {1: "stride s + 1", 2: "clamp to edge", 3: "kc not scaled per pass", 4: "taps in reverse order",
           5: "demodulation threshold ignored"}
MIN_INSIDE = 0.05                                       # of the evaluated taps, per weight term
# (W, H, passes): the shapes at which a tile kernel goes wrong
SHAPES = ((1, 1, 3), (1, 40, 3), (3, 2, 3), (16, 16, 3), (37, 23, 3), (70, 45, 3), (13, 50, 5), (129, 65, 8))
POWERS = (0, 7)
SIGMA_COLOR, SIGMA_POSITION = 2.0, 0.5                  # of the parity cases: chosen so that check_condition holds


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the driver -------------------------------------------------------------------
def build_driver(mutant=0) -> str:
    lib = os.path.join(_HERE, "libdenoise_driver.so" if mutant == 0 else f"libdenoise_driver_m{mutant}.so")
    srcs = [_DRIVER_SRC, os.path.join(sf._ORACLE, "Makefile")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(s) for s in srcs):
        tmp = f"{lib}.tmp{os.getpid()}"
        cmd = [os.environ.get("CC", "gcc")] + sf.oracle_cflags() + [f"-DMUTANT={mutant}", "-shared", "-o", tmp, _DRIVER_SRC]
        subprocess.run(cmd, check=True)
        os.replace(tmp, lib)
    return lib


@functools.lru_cache(maxsize=None)
def driver(mutant=0):
    L = ctypes.CDLL(build_driver(mutant))
    vp, u = ctypes.c_void_p, ctypes.c_uint32
    L.denoise_driver.restype = ctypes.c_int
    L.denoise_driver.argtypes = [vp, vp, u, u, u, u, u, ctypes.c_float, ctypes.c_float, vp, vp]
    return L


def filtered(color, guides, w, h, passes, demodulate=True, m=0, sigma_color=SIGMA_COLOR, sigma_position=SIGMA_POSITION,
             mutant=0, stats=None) -> np.ndarray:
    """[h, w, 4] float32: the yardstick's result.  stats: a float64[4] the
    driver adds to (taps evaluated; taps with wn, wp, wc inside (0.01, 0.99))."""
    c = np.ascontiguousarray(color, np.float32).reshape(h, w, 4)
    g = np.ascontiguousarray(guides, np.uint32).reshape(h * w, sf.WORDS)
    out = np.empty_like(c)
    err = driver(mutant).denoise_driver(c.ctypes.data, g.ctypes.data, w, h, passes, DEMODULATE if demodulate else 0, m,
                                        sigma_color, sigma_position, out.ctypes.data,
                                        None if stats is None else stats.ctypes.data)
    assert err == 0, err
    return out


# ---- synthetic grids -----------------------------------------------------------------
def records(position, normal, albedo, kind=sf.MESH) -> np.ndarray:
    """[n, 28] uint32 records with these positions, normals, albedos and kinds;
    every other word as vrhip_trace_surface leaves it on a diffuse hit or 0."""
    n = len(position)
    rec = np.zeros((n, sf.WORDS), np.uint32)
    rec[:, sf.T] = u32(np.full(n, 1.0))
    rec[:, sf.KIND] = kind
    rec[:, sf.TYPE] = 1
    rec[:, sf.POSITION] = u32(position)
    rec[:, sf.NORMAL] = u32(normal)
    rec[:, sf.COLOR] = u32(albedo)
    return rec


@functools.lru_cache(maxsize=None)
def grid(w, h):
    """(color [h, w, 4] float32, guides [h w, 28] uint32) of the synthetic
    w x h grid, never written."""
    rng = np.random.default_rng(20250000 + 1000 * w + h)
    n = w * h
    y, x = np.divmod(np.arange(n), w)
    region = (x * 3 // w + y * 2 // h) % 3
    if n < 64:                                              # a tiny grid is one region with mild noise: at m = 7 its few
        region = np.zeros(n, np.int64)                      # neighbours must still weigh something
    base = np.array([(0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (0.0, 0.6, 0.8)])[region]
    amp = 10.0 ** rng.uniform(-1.6, -0.1 if n >= 64 else -0.9, (n, 1))
    nrm = base + amp * rng.normal(0.0, 1.0, (n, 3))
    nrm /= np.sqrt((nrm * nrm).sum(-1, keepdims=True))
    z = 0.3 * np.sin(0.7 * x) + 0.2 * np.cos(0.45 * y) + region * 0.8 + rng.normal(0.0, 0.15, n)
    pos = np.stack([x * 0.25, y * 0.25, z], -1)
    alb = rng.uniform(0.1, 1.0, (n, 3))
    special = rng.integers(0, 8, (n, 3))                    # one channel in eight each: 0, the threshold, its next float up
    alb = np.where(special == 0, 0.0, alb).astype(np.float32)
    alb = np.where(special == 1, np.float32(2.0 ** -8), alb)
    alb = np.where(special == 2, np.nextafter(np.float32(2.0 ** -8), np.float32(1.0)), alb).astype(np.float32)
    kind = rng.integers(1, 5, n).astype(np.uint32)
    bad = rng.integers(0, 8, n) == 0
    if n == 1:
        bad[:] = False
    else:
        bad[rng.integers(0, n)] = True                      # at least one invalid cell in every grid but 1 x 1
        bad[(np.flatnonzero(bad)[0] + 1) % n] = False       # and at least one valid one
    kind[bad] = np.array([0, 5, 0xFFFFFFFF], np.uint32)[rng.integers(0, 3, int(bad.sum()))]
    rec = records(pos.astype(np.float32), nrm.astype(np.float32), alb, kind)
    light = 0.5 + 0.5 * np.sin(0.3 * x + 0.2 * y)[:, None] + region[:, None] * 0.7
    col = (np.maximum(alb, 0.05) * light * rng.uniform(0.3, 1.7, (n, 3))).astype(np.float32)
    color = np.concatenate([col, rng.uniform(0.0, 1.0, (n, 1)).astype(np.float32)], -1).reshape(h, w, 4)
    color = np.ascontiguousarray(color, np.float32)
    for a in (color, rec):
        a.setflags(write=False)
    return color, rec


def cases():
    """Every parity case: (w, h, passes, demodulate, m)."""
    return [(w, h, p, demod, m) for (w, h, p) in SHAPES for demod in (False, True) for m in POWERS]


def case_id(c):
    w, h, p, demod, m = c
    return f"{w}x{h}-p{p}-{'demod' if demod else 'plain'}-m{m}"


@functools.lru_cache(maxsize=None)
def reference(w, h, passes, demodulate, m, mutant=0):
    """(result [h, w, 4], stats [4]) of a parity case under the yardstick (or a
    mutant of it): computed once, shared, never written."""
    color, rec = grid(w, h)
    stats = np.zeros(4, np.float64)
    out = filtered(color, rec, w, h, passes, demodulate, m, mutant=mutant, stats=stats)
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


def check_condition(c) -> dict:
    """Each of wn, wp, wc strictly inside (0.01, 0.99) on at least MIN_INSIDE
    of the case's evaluated taps (the 1 x 1 grid is exempt: see the head of
    the file).  Returns the fractions."""
    _, stats = reference(*c)
    frac = {k: float(stats[i + 1] / max(stats[0], 1.0)) for i, k in enumerate(("wn", "wp", "wc"))}
    if (c[0], c[1]) != (1, 1):
        assert stats[0] > 0 and min(frac.values()) >= MIN_INSIDE, f"{case_id(c)}: {frac} of {int(stats[0])} taps"
    return frac


# what each mutant can change: the cases that claim to cover it
def covers(c, mutant) -> bool:
    w, h, p, demod, m = c
    if (w, h) == (1, 1):
        return mutant == 5 and demod          # one cell: no neighbour, no stride, no order
    if mutant == 5:
        return demod
    if mutant == 3:
        return p >= 2
    return True


def same_or_nan_in_both(got, want) -> np.ndarray:
    """Per cell: every channel equal bit for bit, or NaN in both."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return ((u32(got) == u32(want)) | (np.isnan(got) & np.isnan(want))).all(-1)


# ---- rendered views (usefulness, the default parameters) ----------------------------------------------
VIEW_NAMES = ("cornell+mesh", "mesh+tex_d+tex_n+tex_s")      # the Cornell and the HDRI scene with a mesh of surface_cases
VIEW_W, VIEW_H, CONVERGED_FRAMES = 64, 48, 256


@functools.lru_cache(maxsize=None)
def view(name):
    """(noisy [H, W, 4], converged [H, W, 4], guides [H W, 28]) of a 64 x 48
    view of scene `name`: 1 frame, the mean of 256 frames, and the surface
    yardstick's records on the camera rays.  Oracle renders, portable libm."""
    import pyoracle as po
    import radiance_cases as rc
    po.build()
    sc = dict(sf.scene_named(name), width=VIEW_W, height=VIEW_H)
    times = [rc.TIME + i for i in range(CONVERGED_FRAMES)]
    noisy = po.render(sc, frames=1, times=times[:1], libm=po.LIBM_PORTABLE)[0]
    conv = po.render(sc, frames=CONVERGED_FRAMES, times=times, libm=po.LIBM_PORTABLE)[0]
    conv = conv.copy()
    conv[..., :3] *= np.float32(1.0) / np.float32(CONVERGED_FRAMES)
    d = rc.camera_dirs(sc)
    o = np.tile(np.asarray(sc["camera"]["origin"], np.float32), (len(d), 1))
    rec = sf.yardstick(sc, o, d)
    for a in (noisy, conv, rec):
        a.setflags(write=False)
    return noisy, conv, rec


def rmse(a, b) -> float:
    d = np.asarray(a, np.float64)[..., :3] - np.asarray(b, np.float64)[..., :3]
    d = d[np.isfinite(d).all(-1)]
    return float(np.sqrt((d * d).mean()))
