"""Records, edits and the yardstick shared by the tests of
vrhip_shade_surface (test_shade_cpu.py, test_gpu_shade.py).

The yardstick is tests/shade_driver.c: the oracle's trace restated with one
change, the hit and the hit flag of bounce 0 given by the caller.  It includes
oracle/vro.c, so everything from bounce 1 on is the oracle's own code, and
test_shade_cpu.py pins the restatement to the reference-pinned trace: on the
surface oracle's own records (surface_cases.reference) it returns
radiance_cases.oracle_paths' rgb bit for bit.  A path's w is 0: there is no
camera origin and so no depth term.

Records are the (n, 28) uint32 words of vrhip_surface_hit.  The surface
oracle's records are taken whole (surface_cases.reference: oracle_hits plus the
words the call does not read); the driver and the library read kind (0 a miss),
type and the xyz of the six vectors.

Ray sets A to D are surface_cases'.  Seeds: the sets' own for A and B, a fixed
generator for C and D.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
import subprocess

import numpy as np

import pyoracle as po
import radiance_cases as rc
import shading_cases as sh
import surface_cases as sf

_HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = os.path.dirname(os.path.abspath(po.__file__))
_DRIVER_SRC = os.path.join(_HERE, "shade_driver.c")
_DRIVER_LIB = os.path.join(_HERE, "libshade_driver.so")

K_MAX = 5                           # paths per record the shared references hold
SAMPLES = (1, 2, 5)
CPU_PATHS = 3                       # paths per record test_shade_cpu.py compares
MAX_DROPPED = rc.MAX_DROPPED        # of a set's records may be non-finite under the yardstick
MIN_LIT = 0.90                      # of a Cornell scene's lightmap records are non-zero
EDITS = ("unchanged", "lightmap", "type0", "type2", "specular1", "emissive", "miss", "lightmap_flipped")


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def nan_case(name) -> bool:
    """Scenes whose radiance holds NaNs by the reference's own arithmetic:
    every record is kept and a channel must be equal or NaN in both."""
    return name in sh.NAN_CASES


# ---- the driver -------------------------------------------------------------------
def build_driver() -> str:
    srcs = [_DRIVER_SRC, os.path.join(_ORACLE, "vro.c"), os.path.join(_ORACLE, "vro_math.c"),
            os.path.join(_ORACLE, "vro.h"), os.path.join(_ORACLE, "vro_math.h"), os.path.join(_ORACLE, "Makefile")]
    if not os.path.exists(_DRIVER_LIB) or os.path.getmtime(_DRIVER_LIB) < max(os.path.getmtime(s) for s in srcs):
        tmp = f"{_DRIVER_LIB}.tmp{os.getpid()}"
        cmd = [os.environ.get("CC", "gcc")] + sf.oracle_cflags() + ["-Wno-unused-function", "-I", _ORACLE, "-shared", "-o", tmp,
                                                                    _DRIVER_SRC, os.path.join(_ORACLE, "vro_math.c"), "-lm"]
        subprocess.run(cmd, check=True)
        os.replace(tmp, _DRIVER_LIB)
    return _DRIVER_LIB


@functools.lru_cache(maxsize=None)
def driver():
    L = ctypes.CDLL(build_driver())
    vp = ctypes.c_void_p
    L.shade_driver.restype = ctypes.c_int
    L.shade_driver.argtypes = [ctypes.POINTER(po.VroScene), vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp]
    return L


def driver_paths(scene, records, dirs, seeds, k_max) -> np.ndarray:
    """[n, k_max, 4]: path k of record i under the yardstick, portable libm."""
    osc = po.OracleScene(scene, libm=po.LIBM_PORTABLE)
    rec = np.ascontiguousarray(records, np.uint32)
    d = np.ascontiguousarray(dirs, np.float32)
    s = np.ascontiguousarray(seeds, np.uint32)
    n = len(rec)
    assert rec.shape == (n, sf.WORDS) and d.shape == (n, 3) and s.shape == (n, 2)
    out = np.zeros((n, k_max, 4), np.float32)
    err = driver().shade_driver(ctypes.byref(osc.s), rec.ctypes.data, d.ctypes.data, s.ctypes.data, n, k_max,
                                out.ctypes.data)
    assert err == 0, err
    return out


def result_of(paths, n_samples) -> np.ndarray:
    """What vrhip_shade_surface returns for a record's paths: rgb =
    ((0 + r_0 * c) + r_1 * c) + ... in fp32, w = 0."""
    out = rc.record_of(paths, n_samples)
    out[:, 3] = 0.0
    return out


# ---- rays and seeds ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _drawn_seeds(which):
    n = {"C": 512, "D": 64}[which]
    s = np.random.default_rng({"C": 20241020, "D": 20241021}[which]).integers(0, 2**32, (n, 2), dtype=np.uint64)
    s = np.ascontiguousarray(s.astype(np.uint32))
    s.setflags(write=False)
    return s


def ray_set(which, scene=None):
    """(origins, dirs, seeds) of set `which`, never written."""
    o, d = sf.ray_set(which, scene)
    s = rc.ray_set(which)[2] if which in ("A", "B") else _drawn_seeds(which)
    assert len(s) == len(o)
    return o, d, s


# ---- edits ------------------------------------------------------------------------------
def _set3(rec, rows, field, xyz):
    rec[rows, field] = u32(np.asarray(xyz, np.float32))[None, :]


def lightmap(rec, rows=None) -> np.ndarray:
    """The records made into what a lightmap texel is: type 1, colour 1,
    specular 0, emission 0, on hit records only (a record keeps its hit or miss)."""
    out = np.array(rec, np.uint32)
    hit = out[:, sf.KIND] != sf.NONE
    if rows is not None:
        hit &= rows
    out[hit, sf.TYPE] = 1
    _set3(out, hit, sf.COLOR, (1, 1, 1))
    _set3(out, hit, sf.SPECULAR, (0, 0, 0))
    _set3(out, hit, sf.EMISSION, (0, 0, 0))
    return out


def mixed(rec) -> np.ndarray:
    """Set M: the eight edits of EDITS in rotation over the records, applied
    to hit records only."""
    rec = np.asarray(rec, np.uint32)
    out = rec.copy()
    hit = rec[:, sf.KIND] != sf.NONE
    e = np.arange(len(rec)) % len(EDITS)
    out = lightmap(out, hit & ((e == 1) | (e == 7)))
    out[hit & (e == 2), sf.TYPE] = 0
    out[hit & (e == 3), sf.TYPE] = 2
    _set3(out, hit & (e == 4), sf.SPECULAR, (1, 1, 1))
    _set3(out, hit & (e == 5), sf.EMISSION, (0.5, 1, 2))
    _set3(out, hit & (e == 5), sf.COLOR, (2, 0.5, 0))
    m = hit & (e == 6)
    out[m] = 0
    out[m, sf.T] = u32(sf.NO_HIT)
    out[m, sf.PRIM] = sf.MISS
    m = hit & (e == 7)
    out[m, sf.NORMAL] ^= np.uint32(0x80000000)
    return out


def miss_made_a_hit(rec) -> np.ndarray:
    """One record, a miss of `rec` made into a diffuse hit: every vector is
    zero, the normal too, so its radiance is NaN by definition."""
    rec = np.asarray(rec, np.uint32)
    i = int(np.flatnonzero(rec[:, sf.KIND] == sf.NONE)[0])
    out = rec[i:i + 1].copy()
    out[0, sf.KIND], out[0, sf.TYPE] = sf.MESH, 1
    return out, i


def finite(paths) -> np.ndarray:
    return np.isfinite(paths).all(tuple(range(1, np.ndim(paths))))


def kept(paths, cap=MAX_DROPPED) -> np.ndarray:
    ok = finite(paths)
    assert (~ok).sum() <= cap * len(ok), f"{(~ok).sum()} of {len(ok)} records are not finite under the yardstick"
    return ok


def same_or_nan_in_both(got, want) -> np.ndarray:
    return rc.same_or_nan_in_both(got, want)


# ---- shared references ----------------------------------------------------------------------
RECORDS = {"unedited": lambda rec: np.array(rec, np.uint32), "lightmap": lightmap, "mixed": mixed}


@functools.lru_cache(maxsize=None)
def reference(name, which, what="unedited", mesh="shallow"):
    """(records [n, 28] uint32, dirs, seeds, paths [n, K_MAX, 4], kept [n]) of
    scene `name` on ray set `which`, the surface oracle's records edited as
    `what` says: computed once, shared by every test that needs it, never
    written.  In a NaN case every record is kept."""
    po.build()
    sc = sf.scene_named(name, mesh)
    o, d, s = ray_set(which, sc)
    rec = RECORDS[what](sf.reference(name, which, mesh)[0])
    paths = driver_paths(sc, rec, d, s, K_MAX)
    ok = np.ones(len(rec), bool) if nan_case(name) else kept(paths)
    for a in (rec, paths, ok):
        a.setflags(write=False)
    return rec, d, s, paths, ok


def slice_length() -> int:
    """kShadeSlice of vr_shade.hpp: the records a wave takes at a time."""
    from vrenderer_pathtracer_amd import build
    with open(os.path.join(build.CSRC, "vr_shade.hpp")) as f:
        m = re.search(r"^constexpr uint32_t kShadeSlice = (\d+);$", f.read(), re.M)
    return int(m.group(1))
