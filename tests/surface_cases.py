"""Rays, scenes and the yardstick shared by the surface-query tests
(test_surface_cpu.py, test_gpu_surface.py; vrhip_trace_surface).

The yardstick is the oracle's own intersect_scene: tests/surface_driver.c
includes oracle/vro.c and calls the static function on arbitrary rays, with a
hit_t of zeros and the direction normalised by normalize4, in portable-libm
mode.  That gives position, normal, tangent, color, specular, emission and
type.  What was hit and where along the ray the oracle's function does not
return; they are restated:
  spheres  (kind, index, t) of the closest sphere by the driver's copy of the
           selection loops over the oracle's own sphere_intersect;
  mesh     (scenes that show their mesh) the product's host walk
           flat_trace_rays(flat, o, normalised d, tmax = the sphere's t or
           1e20), itself pinned to the reference fixtures: t, prim and the
           barycentrics; a mesh hit replaces the sphere;
  uv       (b0 * uv0 + u * uv1) + v * uv2 in numpy float32.

Ray sets: the radiance tests' A (camera rays) and B (random rays), C (rays
aimed at the scene's mesh, where it shows one) and D.  D exists because A, B
and C together reach the two small spheres with 8 to 19 rays (B with none) and
leave a Cornell box through its open front with 2: 40 of its 64 rays are aimed
at the small spheres and 24 start in front of the scene and point away from
it, so that every kind a scene can produce, a miss included, occurs at least
MIN_KIND times over the scene's sets.

Non-finite records.  At most MAX_DROPPED of a set's records may hold a
non-finite float, and those are not compared.  Two kinds of scene are exempt,
and there every ray is compared, a word equal or NaN in both: the shading
cases whose NaNs are the point (shading_cases.NAN_CASES), and those whose mesh
has zero tangents (ZERO_TANGENT_CASES): there the reference's own
normalize(0) makes the tangent of every mesh hit NaN -- the record carries the
tangent, the radiance never shows it -- and nothing else is.
test_surface_cpu.py ties the restated t to the oracle's hitPoint and the record
to the reference-pinned renders.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
import subprocess

import numpy as np

import flag_lattice as fl
import pyoracle as po
import radiance_cases as rc
import shading_cases as sh

_HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = os.path.dirname(os.path.abspath(po.__file__))
_DRIVER_SRC = os.path.join(_HERE, "surface_driver.c")
_DRIVER_LIB = os.path.join(_HERE, "libsurface_driver.so")

NONE, CORNELL, SMALL, EXAMPLE, MESH = range(5)           # VRHIP_SURF_*
KIND_NAMES = ("none", "cornell", "small", "example", "mesh")
MISS = 0xFFFFFFFF                                        # VRHIP_RAY_MISS
NO_HIT = np.float32(1e20)
WORDS = 28
# words of the record (uint32 / float32 columns)
T, KIND, PRIM, TYPE = 0, 1, 2, 3
POSITION, NORMAL, TANGENT, COLOR, SPECULAR, EMISSION = (slice(4 * k, 4 * k + 3) for k in range(1, 7))
BARY_U, BARY_V, PAD0, TEX_U, TEX_V, PAD1 = 7, 11, 15, 19, 23, 27

COMBO_NAMES = rc.COMBO_NAMES
SHADING_NAMES = rc.SHADING_NAMES
MAX_DROPPED = rc.MAX_DROPPED       # of a set's oracle records may be non-finite
MIN_KIND = 16                      # every kind a scene can produce, over its sets
MIN_MESH_C = 400                   # rays of set C that reach the mesh
ZERO_TANGENT_CASES = tuple(n for n in rc.SHADING_NAMES if sh.CASES[n].get("mesh") == "tan0")


def nan_case(name) -> bool:
    """Scenes in which every ray is kept and a word must be equal or NaN in both."""
    return name in sh.NAN_CASES or name in ZERO_TANGENT_CASES


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the driver -------------------------------------------------------------------
def oracle_cflags():
    """CFLAGS of oracle/Makefile, as written there."""
    with open(os.path.join(_ORACLE, "Makefile")) as f:
        m = re.search(r"^CFLAGS\s*:=\s*(.*)$", f.read(), re.M)
    return m.group(1).split()


def build_driver() -> str:
    srcs = [_DRIVER_SRC, os.path.join(_ORACLE, "vro.c"), os.path.join(_ORACLE, "vro_math.c"),
            os.path.join(_ORACLE, "vro.h"), os.path.join(_ORACLE, "vro_math.h"), os.path.join(_ORACLE, "Makefile")]
    if not os.path.exists(_DRIVER_LIB) or os.path.getmtime(_DRIVER_LIB) < max(os.path.getmtime(s) for s in srcs):
        tmp = f"{_DRIVER_LIB}.tmp{os.getpid()}"
        cmd = [os.environ.get("CC", "gcc")] + oracle_cflags() + ["-Wno-unused-function", "-I", _ORACLE, "-shared", "-o", tmp,
                                                                 _DRIVER_SRC, os.path.join(_ORACLE, "vro_math.c"), "-lm"]
        subprocess.run(cmd, check=True)
        os.replace(tmp, _DRIVER_LIB)
    return _DRIVER_LIB


@functools.lru_cache(maxsize=None)
def driver():
    L = ctypes.CDLL(build_driver())
    vp = ctypes.c_void_p
    L.surface_driver.restype = ctypes.c_int
    L.surface_driver.argtypes = [ctypes.POINTER(po.VroScene), vp, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    L.surface_driver_sphere.restype = None
    L.surface_driver_sphere.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp]
    return L


def sphere_of(kind, index):
    """(color [3], emission [3]) of the oracle's sphere (kind, index)."""
    c, e = np.zeros(3, np.float32), np.zeros(3, np.float32)
    driver().surface_driver_sphere(int(kind), int(index), c.ctypes.data, e.ctypes.data)
    return c, e


def normalised(dirs) -> np.ndarray:
    """normalize4 in numpy float32: d * (1 / sqrt((x x + y y) + z z))."""
    d = np.ascontiguousarray(dirs, np.float32)
    with np.errstate(all="ignore"):
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inv = np.float32(1.0) / np.sqrt(dd)
        out = d * inv[:, None]
    assert out.dtype == np.float32
    return np.ascontiguousarray(out)


def oracle_hits(scene, origins, dirs) -> dict:
    """What the driver returns for these rays: hit [n] bool, rows [n, 6, 4]
    (hitPoint, normal, tangent, emission, color, spec), type [n], and the
    closest sphere's kind, index and t."""
    osc = po.OracleScene(scene, libm=po.LIBM_PORTABLE)
    o = np.ascontiguousarray(origins, np.float32)
    d = np.ascontiguousarray(dirs, np.float32)
    n = len(o)
    rows = np.zeros((n, 6, 4), np.float32)
    types = np.zeros(n, np.uint32)
    hit, kind, index = (np.zeros(n, np.int32) for _ in range(3))
    st = np.zeros(n, np.float32)
    err = driver().surface_driver(ctypes.byref(osc.s), o.ctypes.data, d.ctypes.data, n, rows.ctypes.data, types.ctypes.data,
                                  hit.ctypes.data, kind.ctypes.data, index.ctypes.data, st.ctypes.data)
    assert err == 0, err
    return dict(hit=hit != 0, rows=rows, type=types, kind=kind, index=index, sphere_t=st)


def shows_mesh(scene) -> bool:
    return scene.get("mesh_flat") is not None and not scene.get("example_sphere")


def yardstick(scene, origins, dirs) -> np.ndarray:
    """[n, 28] uint32: the records vrhip_trace_surface must return for a
    scene whose mesh was uploaded as scene["mesh_flat"] (prim: the slot of the
    triangle's first vertex)."""
    from vrenderer_pathtracer_amd import flat_trace_rays
    o = np.ascontiguousarray(origins, np.float32)
    h = oracle_hits(scene, o, dirs)
    n = len(o)
    t = h["sphere_t"].copy()
    kind = h["kind"].astype(np.uint32)
    prim = h["index"].astype(np.uint32)
    bary = np.zeros((n, 2), np.float32)
    uv = np.zeros((n, 2), np.float32)
    if shows_mesh(scene):
        flat = scene["mesh_flat"]
        w = flat_trace_rays(flat, o, normalised(dirs), t)
        m = w["prim"] >= 0
        t[m] = w["t"][m]
        kind[m] = MESH
        prim[m] = w["prim"][m].astype(np.uint32)
        bary[m, 0], bary[m, 1] = w["u"][m], w["v"][m]
        a = w["prim"][m]
        uvs = np.ascontiguousarray(flat["uvs"], np.float32).reshape(-1, 2)
        bu, bv = bary[m, 0:1], bary[m, 1:2]
        with np.errstate(all="ignore"):
            b0 = np.float32(1.0) - bu - bv
            uv[m] = (b0 * uvs[a] + bu * uvs[a + 1]) + bv * uvs[a + 2]
        assert uv.dtype == np.float32
    hit = kind != NONE
    assert (hit == h["hit"]).all(), "the restated closest hit and the oracle's return value disagree on hit or miss"
    assert (t[~hit] == NO_HIT).all()
    rec = np.zeros((n, WORDS), np.uint32)
    rec[:, T] = u32(t)
    rec[:, KIND] = kind
    rec[:, PRIM] = np.where(hit, prim, np.uint32(MISS))
    rec[:, TYPE] = h["type"]
    for field, row in ((POSITION, 0), (NORMAL, 1), (TANGENT, 2), (EMISSION, 3), (COLOR, 4), (SPECULAR, 5)):
        rec[:, field] = u32(h["rows"][:, row, :3])
    rec[:, BARY_U], rec[:, BARY_V] = u32(bary[:, 0]), u32(bary[:, 1])
    rec[:, TEX_U], rec[:, TEX_V] = u32(uv[:, 0]), u32(uv[:, 1])
    rec[~hit, 1 + T:] = 0
    rec[~hit, KIND] = NONE
    rec[~hit, PRIM] = MISS
    return rec


def floats(rec) -> np.ndarray:
    return np.ascontiguousarray(rec, np.uint32).view(np.float32)


def finite(rec) -> np.ndarray:
    """Per record: every float word finite (the integer words are not floats)."""
    f = floats(rec).copy()
    f[:, [KIND, PRIM, TYPE]] = 0.0
    return np.isfinite(f).all(-1)


def kept(rec) -> np.ndarray:
    ok = finite(rec)
    assert (~ok).sum() <= MAX_DROPPED * len(ok), f"{(~ok).sum()} of {len(ok)} rays have a non-finite oracle record"
    return ok


def same_or_nan_in_both(got, want) -> np.ndarray:
    """Per record: every word equal, or a float word NaN in both."""
    got, want = np.ascontiguousarray(got, np.uint32), np.ascontiguousarray(want, np.uint32)
    fg, fw = floats(got), floats(want)
    nan = np.isnan(fg) & np.isnan(fw)
    nan[:, [KIND, PRIM, TYPE]] = False
    return ((got == want) | nan).all(-1)


# ---- rays ---------------------------------------------------------------------------
def triangles_of(flat) -> np.ndarray:
    """[n_tris, 3, 3]: the triangles of a flattened mesh, in slot order (a
    terminator slot has x = -0)."""
    v = np.ascontiguousarray(flat["verts"], np.float32).reshape(-1, 4)
    term = v[:, 0].view(np.uint32) == 0x80000000
    first, i, n = [], 0, len(v)
    while i < n:
        if term[i]:
            i += 1
        else:
            first.append(i)
            i += 3
    first = np.asarray(first, np.int64)
    return np.stack([v[first, :3], v[first + 1, :3], v[first + 2, :3]], 1)


def aimed_rays(flat, n=512, seed=20240611):
    """Set C for a mesh: origins uniform in [-40, 40]^3, each aimed at a
    random barycentric point of a random triangle, the direction scaled to a
    length in [0.1, 10]."""
    tris = triangles_of(flat).astype(np.float64)
    rng = np.random.default_rng(seed)
    o = rng.uniform(-40.0, 40.0, (n, 3)).astype(np.float32)
    tri = tris[rng.integers(0, len(tris), n)]
    b = rng.dirichlet((1.0, 1.0, 1.0), n)
    target = (tri * b[:, :, None]).sum(1)
    v = target - o.astype(np.float64)
    v /= np.sqrt((v * v).sum(-1, keepdims=True))
    d = (v * rng.uniform(0.1, 10.0, (n, 1))).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def extra_rays(seed=20240612):
    """Set D: 40 rays from points uniform in [-40, 40]^3 aimed at a random
    point inside one of the two small spheres (centres (15, 0, 15) and
    (25, 0, 15), radius 3.5), and 24 from points with z in [20, 40] that point
    towards +z within a slope of 0.005, out of the Cornell box's open front
    (its side walls are spheres of radius 1e5 that a steeper ray meets further
    out: the wall at x = 50 + z^2 / 2e5); lengths in [0.1, 10]."""
    rng = np.random.default_rng(seed)
    n_s, n_e = 40, 24
    o = rng.uniform(-40.0, 40.0, (n_s + n_e, 3))
    centre = np.where((np.arange(n_s) % 2 == 0)[:, None], (15.0, 0.0, 15.0), (25.0, 0.0, 15.0))
    v = centre + rng.uniform(-2.0, 2.0, (n_s, 3)) - o[:n_s]
    o[n_s:, 2] = rng.uniform(20.0, 40.0, n_e)
    e = np.concatenate([rng.uniform(-0.005, 0.005, (n_e, 2)), np.ones((n_e, 1))], -1)
    v = np.concatenate([v, e])
    v /= np.sqrt((v * v).sum(-1, keepdims=True))
    d = (v * rng.uniform(0.1, 10.0, (len(v), 1))).astype(np.float32)
    return np.ascontiguousarray(o.astype(np.float32)), np.ascontiguousarray(d)


_MESHES = {}          # id(flat) -> set C, for the shared, never-written meshes of fl.mesh_of and sh.mesh_of


def ray_set(which, scene=None):
    """(origins [n,3], dirs [n,3]), never written.  A and B: the radiance
    tests' 1,024 camera rays and 512 random rays.  C: 512 rays aimed at the
    scene's mesh.  D: 64 rays at the small spheres and out of the scene."""
    if which in ("A", "B"):
        return rc.ray_set(which)[:2]
    if which == "D":
        if "D" not in _MESHES:
            out = extra_rays()
            for a in out:
                a.setflags(write=False)
            _MESHES["D"] = (None, out)
        return _MESHES["D"][1]
    assert which == "C" and shows_mesh(scene)
    flat = scene["mesh_flat"]
    key = id(flat["verts"])
    if key not in _MESHES:
        out = aimed_rays(flat)
        for a in out:
            a.setflags(write=False)
        _MESHES[key] = (flat["verts"], out)               # the array is held, so its id stays its own
    return _MESHES[key][1]


def sets_of(scene):
    return ("A", "B", "C", "D") if shows_mesh(scene) else ("A", "B", "D")


def kinds_of(scene):
    """The kinds the scene can produce."""
    k = [NONE, SMALL]
    if scene.get("cornell"):
        k.append(CORNELL)
    if scene.get("example_sphere"):
        k.append(EXAMPLE)
    if shows_mesh(scene):
        k.append(MESH)
    return tuple(sorted(k))


# ---- shared references -------------------------------------------------------------------
def scene_named(name, mesh="shallow") -> dict:
    if name in sh.CASES:
        return sh.make_case(name)
    return fl.scene_of(rc.combo_of(name), mesh)


@functools.lru_cache(maxsize=None)
def reference(name, which, mesh="shallow"):
    """(records [n, 28] uint32, kept [n]) of scene `name` on ray set `which`:
    computed once, shared by every test that needs it, never written.  In a
    NaN case (nan_case) every ray is kept."""
    po.build()
    sc = scene_named(name, mesh)
    o, d = ray_set(which, sc)
    rec = yardstick(sc, o, d)
    ok = np.ones(len(rec), bool) if nan_case(name) else kept(rec)
    rec.setflags(write=False)
    ok.setflags(write=False)
    return rec, ok


def check_coverage(name, mesh="shallow") -> dict:
    """The conditions on the yardstick itself; returns the counts per kind
    over the scene's sets."""
    sc = scene_named(name, mesh)
    counts = np.zeros(5, np.int64)
    for which in sets_of(sc):
        rec, ok = reference(name, which, mesh)
        counts += np.bincount(rec[:, KIND], minlength=5)[:5]
        if which == "C":
            assert (rec[:, KIND] == MESH).sum() >= MIN_MESH_C, f"{name}: {(rec[:, KIND] == MESH).sum()} rays of C hit the mesh"
    for k in kinds_of(sc):
        assert counts[k] >= MIN_KIND, f"{name}: kind {KIND_NAMES[k]} occurs {counts[k]} times over its sets"
    return {KIND_NAMES[k]: int(counts[k]) for k in range(5)}
