"""Meshes, scenes and the yardstick shared by the atlas tests
(test_atlas_cpu.py, test_gpu_atlas.py; vrhip_surface_at, vrhip_atlas_surface).

The yardstick is tests/atlas_driver.c, which includes oracle/vro.c:
  at(scene, slots, bary)     the oracle's own leaf_hit at (slot, u, v), the hit
                             point overwritten with the barycentric position;
  raster(scene, W, H, g)     the definition of include/vrhip.h restated in
                             plain C, brute force over all triangles per texel
                             (box=True: triangle by triangle over a bounding
                             box of its own, for the larger cases), the gutter
                             passes, then at() per texel.
Records are [n, 28] uint32 in the word order of surface_cases.  A scene's mesh
is scene["mesh_flat"] and prim is the flat slot of a triangle's first vertex,
as after initMesh; prim_of_slot renames the triangles for device-built meshes
(the winner is the smallest prim in the caller's terms).

Meshes are indexed dicts (positions, normals, tangents, uvs, tris) whose uvs
are the point; the positions are seeded triangles of their own, so that every
triangle is a proper one in space and differs from every other whatever its
uvs are (the chart mesh is a sheet that faces the camera instead).
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np

import pyoracle as po
import shading_cases as sh
import surface_cases as sf

_HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = os.path.dirname(os.path.abspath(po.__file__))
_DRIVER_SRC = os.path.join(_HERE, "atlas_driver.c")
_DRIVER_LIB = os.path.join(_HERE, "libatlas_driver.so")

MISS = sf.MISS
F = np.float32


# ---- the driver -------------------------------------------------------------------
def build_driver() -> str:
    srcs = [_DRIVER_SRC] + [os.path.join(_ORACLE, f) for f in ("vro.c", "vro_math.c", "vro.h", "vro_math.h", "Makefile")]
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
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    sp = ctypes.POINTER(po.VroScene)
    L.atlas_at.restype = None
    L.atlas_at.argtypes = [sp, vp, vp, u32, vp]
    L.atlas_raster.restype = None
    L.atlas_raster.argtypes = [sp, vp, u32, u32, u32, ctypes.c_int, vp]
    L.atlas_first_slots.restype = None
    L.atlas_first_slots.argtypes = [sp, vp]
    L.atlas_tex_addr.restype = ctypes.c_int
    L.atlas_tex_addr.argtypes = [u32, u32, ctypes.c_float, ctypes.c_float]
    return L


def at(scene, slots, bary) -> np.ndarray:
    osc = po.OracleScene(scene, libm=po.LIBM_PORTABLE)
    s = np.ascontiguousarray(slots, np.uint32)
    b = np.ascontiguousarray(bary, np.float32).reshape(-1, 2)
    assert len(s) == len(b)
    rec = np.zeros((len(s), 28), np.uint32)
    driver().atlas_at(ctypes.byref(osc.s), s.ctypes.data, b.ctypes.data, len(s), rec.ctypes.data)
    return rec


def raster(scene, w, h, gutter=0, box=False, prim_of_slot=None) -> np.ndarray:
    osc = po.OracleScene(scene, libm=po.LIBM_PORTABLE)
    rec = np.zeros((w * h, 28), np.uint32)
    pos = None
    if prim_of_slot is not None:
        pos = np.ascontiguousarray(prim_of_slot, np.uint32)
        assert len(pos) == osc.s.n_slots
    driver().atlas_raster(ctypes.byref(osc.s), None if pos is None else pos.ctypes.data, w, h, gutter, int(box), rec.ctypes.data)
    return rec


def first_slots(flat) -> np.ndarray:
    """The slots that are a triangle's first vertex, ascending."""
    v = np.ascontiguousarray(flat["verts"], np.float32).reshape(-1, 4)
    term = v[:, 0].view(np.uint32) == 0x80000000
    out, i = [], 0
    while i < len(v):
        if term[i]:
            i += 1
        else:
            out.append(i)
            i += 3
    return np.asarray(out, np.int64)


def tex_addr(w, h, u, v) -> np.ndarray:
    """The oracle's own tex_addr, element by element."""
    L = driver()
    u, v = np.asarray(u, np.float32).reshape(-1), np.asarray(v, np.float32).reshape(-1)
    return np.asarray([L.atlas_tex_addr(int(w), int(h), float(a), float(b)) for a, b in zip(u, v)], np.int64)


def prim_of_slot(flat, mesh) -> np.ndarray:
    """[n_slots] uint32: the row of mesh["tris"] whose three positions and uvs
    are those of the triangle that starts at each slot (MISS elsewhere)."""
    P = np.ascontiguousarray(mesh["positions"], np.float32)
    U = np.ascontiguousarray(mesh["uvs"], np.float32) if mesh.get("uvs") is not None else np.zeros((len(P), 2), np.float32)
    T = np.asarray(mesh["tris"], np.int64)
    rows = {}
    for k, t in enumerate(T):
        rows.setdefault(P[t].view(np.uint32).tobytes() + U[t].view(np.uint32).tobytes(), k)
    v = np.ascontiguousarray(flat["verts"], np.float32).reshape(-1, 4)[:, :3]
    uv = np.ascontiguousarray(flat["uvs"], np.float32).reshape(-1, 2)
    out = np.full(len(v), MISS, np.uint32)
    for s in first_slots(flat):
        out[s] = rows[np.ascontiguousarray(v[s:s + 3]).view(np.uint32).tobytes() +
                      np.ascontiguousarray(uv[s:s + 3]).view(np.uint32).tobytes()]
    return out


# ---- meshes -----------------------------------------------------------------------
def soup(uvs3, seed=1, planar=False) -> dict:
    """An unshared-vertex mesh from per-triangle uvs [n, 3, 2]: triangle k is
    rows 3k .. 3k + 2.  Positions: a seeded triangle of its own near a seeded
    centre (finite whatever the uvs), or with planar (uvs in [0, 1]) the sheet
    ((u - .5) * 80, (v - .5) * 80, a seeded bump) that faces the default
    camera; unit normals and tangents, seeded."""
    uvs3 = np.asarray(uvs3, np.float32).reshape(-1, 3, 2)
    n = len(uvs3)
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-25.0, 25.0, (n, 1, 3))
    pos = (centre + rng.uniform(-3.0, 3.0, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    if planar:
        sheet = (uvs3.reshape(-1, 2).astype(np.float64) - 0.5) * 80.0
        pos = np.concatenate([sheet, rng.uniform(-1.0, 1.0, (3 * n, 1))], -1).astype(np.float32)
    nrm = rng.normal(0.0, 1.0, (3 * n, 3))
    nrm /= np.sqrt((nrm * nrm).sum(-1, keepdims=True))
    tan = np.cross(nrm, rng.normal(0.0, 1.0, (3 * n, 3)))
    tan /= np.sqrt((tan * tan).sum(-1, keepdims=True))
    return dict(positions=pos, normals=nrm.astype(np.float32), tangents=tan.astype(np.float32),
                uvs=np.ascontiguousarray(uvs3.reshape(-1, 2)), tris=np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))


def quad(swap_order=False, mirrored=False) -> dict:
    """One quad, corners (0,0) (1,0) (1,1) (0,1), split along the diagonal
    (0,0)-(1,1): every centre (i + .5, i + .5) / n of a square atlas lies
    exactly on the edge the two triangles share."""
    c = np.asarray([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32)
    t = [(0, 1, 2), (0, 2, 3)]
    if mirrored:
        t = [(a, c_, b) for a, b, c_ in t]
    if swap_order:
        t = t[::-1]
    return soup(np.stack([c[list(k)] for k in t]), seed=2)


def single_triangle() -> dict:
    return soup([[(0.1, 0.05), (0.9, 0.2), (0.3, 0.95)]], seed=3)


def knot(margin=0.0, uvs=True) -> dict:
    from vrenderer_pathtracer_amd import scenes
    m = scenes.torus_knot_unwrapped(24, 12, margin)
    if not uvs:
        m = dict(m, uvs=None)
    return m


def big_small(big_first, w=300, h=200, n_small=500, seed=4) -> dict:
    """Two triangles that cover the whole atlas and n_small sub-texel and
    few-texel ones on top, the big pair first (it wins everywhere) or last (it
    loses wherever a small one covers a centre)."""
    rng = np.random.default_rng(seed)
    big = np.asarray([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]], np.float64)
    c = rng.uniform(0.0, 1.0, (n_small, 1, 2))
    size = np.where(rng.integers(0, 2, (n_small, 1, 1)) == 0, 0.4, 4.0) / np.asarray([w, h], np.float64)
    small = c + rng.uniform(-1.0, 1.0, (n_small, 3, 2)) * size
    uv = np.concatenate([big, small] if big_first else [small, big])
    return soup(uv, seed=seed)


def hostile() -> dict:
    """uvs partly and wholly outside [0,1]^2, of +-1e9 and +-3e38, denormal,
    NaN and infinite, zero-area and collinear triangles, two coincident
    charts.  The finite proper triangles among them cover a good part of the
    atlas, so a wrong box shows."""
    rng = np.random.default_rng(6)
    t = []
    t += list(rng.uniform(-1.0, 2.0, (40, 3, 2)))                          # partly and wholly outside, in [-1, 2)
    t += [[(-0.5, -0.5), (-0.1, -0.4), (-0.3, -0.1)], [(1.2, 1.1), (1.9, 1.3), (1.5, 1.8)]]     # wholly outside
    for s in (1e9, -1e9, 3e38, -3e38):
        t += [[(0.2, 0.3), (s, 0.4), (0.5, 0.6)], [(s, s), (0.5, 0.1), (0.1, 0.9)], [(s, -s), (-s, s), (0.5, 0.5)],
              [(s, 0.0), (s, 1.0), (0.9 * s, 0.5)]]
    den = np.float32(1e-42)
    t += [[(den, den), (0.4, float(den)), (float(den), 0.4)], [(0.0, 0.0), (float(den), 0.0), (0.0, float(den))],
          [(-float(den), 0.6), (0.3, 0.6), (0.0, 0.9)]]
    for bad in (np.nan, np.inf, -np.inf):
        t += [[(bad, 0.2), (0.8, 0.2), (0.5, 0.8)], [(0.1, 0.1), (0.9, bad), (0.5, 0.9)], [(bad, bad), (bad, bad), (bad, bad)]]
    t += [[(0.3, 0.3), (0.3, 0.3), (0.7, 0.7)], [(0.2, 0.5), (0.2, 0.5), (0.2, 0.5)],       # zero area
          [(0.1, 0.1), (0.5, 0.5), (0.9, 0.9)], [(0.0, 0.25), (0.5, 0.25), (1.0, 0.25)]]    # collinear
    chart = [[(0.55, 0.05), (0.95, 0.05), (0.95, 0.45)], [(0.55, 0.05), (0.95, 0.45), (0.55, 0.45)]]
    t += chart + chart                                                       # two coincident charts
    with np.errstate(all="ignore"):
        return soup(np.asarray(t, np.float64).astype(np.float32), seed=6)


CHART_W, CHART_H = 65, 63
# four axis-aligned rectangles (x0, y0, x1, y1) in texels of the 65 x 63 atlas,
# offset by non-integer amounts, each at least one texel wide: the first two
# are 2.6 texels apart (closer than 2 * gutter from gutter 2 on), the third
# touches the fourth only diagonally (a texel between them is reached only
# through a corner), the fourth is barely more than a texel high
CHARTS = ((3.3, 4.6, 20.7, 18.2), (23.3, 2.4, 40.9, 30.5), (5.5, 30.7, 30.2, 50.4), (31.6, 51.7, 60.4, 53.1))


def chart_mesh() -> dict:
    t = []
    for x0, y0, x1, y1 in CHARTS:
        a, b, c, d = ((x0 / CHART_W, y0 / CHART_H), (x1 / CHART_W, y0 / CHART_H), (x1 / CHART_W, y1 / CHART_H),
                      (x0 / CHART_W, y1 / CHART_H))
        t += [[a, b, c], [a, c, d]]
    return soup(np.asarray(t, np.float64).astype(np.float32), seed=7, planar=True)


def chart_points(n=4000, seed=8):
    """(chart, u, v): n points of the charts in fp32 uv, strictly inside."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(CHARTS), n)
    r = np.asarray(CHARTS, np.float64)[k]
    fx, fy = rng.uniform(0.001, 0.999, n), rng.uniform(0.001, 0.999, n)
    u = ((r[:, 0] + fx * (r[:, 2] - r[:, 0])) / CHART_W).astype(np.float32)
    v = ((r[:, 1] + fy * (r[:, 3] - r[:, 1])) / CHART_H).astype(np.float32)
    return k, u, v


@functools.lru_cache(maxsize=None)
def flat_of(which, *args) -> dict:
    """build_flat of a mesh of this module by name, shared and never written."""
    from vrenderer_pathtracer_amd import build_flat
    mesh = globals()[which](*args)
    m = dict(mesh)
    if m.get("uvs") is None:
        m["uvs"] = np.zeros((len(m["positions"]), 2), np.float32)
    flat = build_flat(m, max_leaf_tris=2)
    for a in flat.values():
        a.setflags(write=False)
    return flat


# ---- scenes -----------------------------------------------------------------------
SCENE_KINDS = ("plain", "maps_odd", "maps_tall", "brdf_view", "tan0")


def scene_of(flat, kind="plain", w=64, h=48) -> dict:
    """An HDRI scene around a flat mesh.  maps_*: every map loaded, in the odd
    shapes of shading_cases (non-square sizes, a single column); brdf_view: the
    maps and the BRDF view; tan0: the maps on a mesh whose tangents are zero
    (the face normal is taken, the record's tangent is normalize(0))."""
    from vrenderer_pathtracer_amd import scenes
    maps = sh.maps_of("tall" if kind == "maps_tall" else "odd")
    sc = dict(camera=scenes.default_camera(), fresnel_coef=0.1, fresnel_pow=3.0, width=w, height=h, time=12345,
              cornell=False, example_sphere=False, view_brdf=kind == "brdf_view", hdr=maps["hdr"], mesh_flat=flat,
              name=f"atlas_{kind}")
    if kind != "plain":
        sc.update({k: maps[k] for k in sh.TEX_KEYS})
    if kind == "tan0":
        sc["mesh_flat"] = dict(flat, tangents=np.zeros_like(flat["tangents"]))
    return sc


def same(got, want, what, nan_ok=False):
    got, want = np.ascontiguousarray(got, np.uint32), np.ascontiguousarray(want, np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = sf.same_or_nan_in_both(got, want) if nan_ok else (got == want).all(-1)
    bad = np.flatnonzero(~ok)
    if len(bad):
        i = bad[0]
        words = np.flatnonzero(got[i] != want[i]).tolist()
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ (first {bad[:8].tolist()}; record {i} words "
                             f"{words}: {got[i, words].tolist()} against {want[i, words].tolist()})")
