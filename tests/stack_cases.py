"""Trees that fill the traversal stack to its last entry, shared by
test_stack_cpu.py, test_gpu_stack.py and the `stacks` family of the
reference-rendered fixtures.

The walk keeps its sentinel in entry 0 and pushes the far child when it enters
both, so a tree of depth D can need D + 1 entries, and the kernels are built
with 16, 24, 32 and 64 entries for depths up to 15, 23, 30 and 62
(vr_ctx.hpp mesh_stack_entries): no slack at 15, 23, 30 and 62.  DEPTHS holds
those and the first depth of each next size.

comb_tree(D): a chain of D inner nodes in chain_tree's layout, node i holding
triangle i as a leaf (child 0) and node i + 1 (child 1), the last node two
leaves.  The triangles lie on planes one behind the other along the z axis,
triangle D nearest the camera, so for a ray down the axis the chain child is
the near one at every level and the leaf is pushed: D pushes.  Every triangle
is a thin wedge laid diagonally across the axis, so its box contains the whole
view cross-section (VIEW) while a ray hits only some of them.  The nearest
triangle is a sliver and its sibling, the far leaf of the last node and the
one entry a stack one short loses, covers the view.

legged_comb_tree(D): the spine's other child is an inner node with two leaves,
and the last spine node holds two of them: D - 1 spine nodes, D legs, 2 D
triangles.  The longest root path, down the spine and into the nearest leg,
pushes at every level; what is popped afterwards are legs, each of which
pushes again.

tie_comb(D, where): a comb with one pair of coincident triangles (their
normals opposite, so the winner shows in a render as well as in `prim`).

The 25 % that the one-short mutant must change (test_stack_cpu.py) is a
condition on these inputs; they are shaped for it: sliver and cover as above,
and five of every eight spine_rays go down the spine.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
import subprocess

import numpy as np

import pyoracle as po
from ray_query_cases import EPS, F, NO_HIT, TERM, _span, brute_force, flat_triangles

DEPTHS = (15, 16, 23, 24, 30, 31, 62)
KINDS = ("comb", "legged")
LEGGED_DEPTHS = (15, 30, 62)         # of the legged comb's GPU cases
TIE_DEPTHS = (30, 62)
SMALL_IMAGES = ((16, 16), (48, 32))  # the small-launch kernels' one-frame calls
W, H = 64, 48
TIMES = (12345, 12346, 12347)       # scene time + k, as the GPU tests' render helpers count
N_QUERY = 256                        # rays of a query case
Z_FAR, Z_NEAR = -30.0, 30.0          # the planes of the farthest and the nearest triangle
REACH = 12.0                         # half the length of a wedge
VIEW = 3.0                           # every leaf box contains [-VIEW, VIEW]^2 at its plane
CAMERA = dict(origin=(0.0, 0.0, 150.0), dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), right=(1.0, 0.0, 0.0), fov_scale=0.015)

_HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = os.path.dirname(os.path.abspath(po.__file__))
_DRIVER_SRC = os.path.join(_HERE, "stack_driver.c")
_DRIVER_LIB = os.path.join(_HERE, "libstack_driver.so")


# ---- triangles -----------------------------------------------------------------------
def _wedge(rng, z, dz, width):
    """A wedge of half-length REACH through a point near the axis, within 25
    degrees of a diagonal, `width` wide at its blunt end, tilted out of its
    plane by at most dz / 4."""
    th = np.deg2rad(rng.choice([45.0, 135.0, 225.0, 315.0]) + rng.uniform(-25.0, 25.0))
    u, n = np.array([np.cos(th), np.sin(th)]), np.array([-np.sin(th), np.cos(th)])
    c = rng.uniform(-1.0, 1.0, 2)
    xy = np.stack([c + REACH * u, c - REACH * u + 0.5 * width * n, c - REACH * u - 0.5 * width * n])
    return np.concatenate([xy, z + rng.uniform(-0.25, 0.25, (3, 1)) * dz], -1)


def _cover(rng, z, dz):
    """A triangle whose inscribed circle (radius 5, centre within 0.5 of the axis) holds the view."""
    c = rng.uniform(-0.5, 0.5, 2)
    a = np.deg2rad(np.array([90.0, 210.0, 330.0]) + rng.uniform(-10.0, 10.0))
    xy = c + 10.0 * np.stack([np.cos(a), np.sin(a)], -1)
    return np.concatenate([xy, z + rng.uniform(-0.25, 0.25, (3, 1)) * dz], -1)


def _triangles(n, seed, tie=None):
    """n triangles (n,3,3) float32 on n planes from Z_FAR to Z_NEAR: wedges,
    the last a sliver and the one before it the cover."""
    rng = np.random.default_rng(seed)
    dz = (Z_NEAR - Z_FAR) / (n - 1)
    V = np.zeros((n, 3, 3))
    for i in range(n):
        z = Z_FAR + dz * i
        if i == n - 1:
            V[i] = _wedge(rng, z, dz, 0.3 if tie is None else 4.0)
        elif i == n - 2:
            V[i] = _cover(rng, z, dz)
        else:
            V[i] = _wedge(rng, z, dz, rng.uniform(1.5, 4.0))
    V = V.astype(np.float32)
    lo, hi = V.min(1), V.max(1)
    assert (lo[:, :2] < -VIEW).all() and (hi[:, :2] > VIEW).all(), "a leaf box does not contain the view"
    assert (lo[1:, 2] > hi[:-1, 2]).all(), "the planes are not in order"
    return V


def _attributes(V, seed):
    """Per slot: the unit face normal towards the camera, a unit tangent along
    the first edge, and drawn uvs; terminator slots zero."""
    rng = np.random.default_rng(seed + 1)
    T = len(V)
    Vd = V.astype(np.float64)
    fn = np.cross(Vd[:, 1] - Vd[:, 0], Vd[:, 2] - Vd[:, 0])
    fn *= np.where(fn[:, 2:3] < 0, -1.0, 1.0) / np.linalg.norm(fn, axis=1, keepdims=True)
    tg = Vd[:, 1] - Vd[:, 0]
    tg /= np.linalg.norm(tg, axis=1, keepdims=True)
    verts, normals, tangents = (np.zeros((4 * T, 4), np.float32) for _ in range(3))
    uvs = np.zeros((4 * T, 2), np.float32)
    for t in range(T):
        verts[4 * t:4 * t + 3, :3] = V[t]
        verts[4 * t + 3, 0] = np.array([TERM], np.uint32).view(np.float32)[0]
        normals[4 * t:4 * t + 3, :3] = fn[t]
        tangents[4 * t:4 * t + 3, :3] = tg[t]
        uvs[4 * t:4 * t + 3] = rng.uniform(0.0, 1.0, (3, 2))
    return verts, normals, tangents, uvs


def _box(P):
    P = P.reshape(-1, 3)
    return P.min(0), P.max(0)


def _node(bvh, i, box0, idx0, box1, idx1):
    (l0, h0), (l1, h1) = box0, box1
    bvh[i, 0] = [l0[0], h0[0], l0[1], h0[1]]
    bvh[i, 1] = [l1[0], h1[0], l1[1], h1[1]]
    bvh[i, 2] = [l0[2], h0[2], l1[2], h1[2]]
    bvh.view(np.int32)[i, 3, :2] = [idx0, idx1]


def _flat(bvh, V, seed):
    verts, normals, tangents, uvs = _attributes(V, seed)
    return dict(bvh=bvh.reshape(-1, 4), verts=verts, normals=normals, tangents=tangents, uvs=uvs)


def _comb(V, depth, seed, swap_last=False):
    bvh = np.zeros((depth, 4, 4), np.float32)
    for i in range(depth):
        last = i + 1 == depth
        a, b = (i + 1, i) if last and swap_last else (i, i + 1)
        _node(bvh, i, _box(V[a]), ~(4 * a), _box(V[b] if last else V[i + 1:]), ~(4 * b) if last else 4 * (i + 1))
    return _flat(bvh, V, seed)


@functools.lru_cache(maxsize=None)
def comb_tree(depth):
    """The comb of `depth` inner nodes and depth + 1 triangles; never written."""
    return _frozen(_comb(_triangles(depth + 1, 100 + depth), depth, 100 + depth))


@functools.lru_cache(maxsize=None)
def legged_comb_tree(depth):
    """depth - 1 spine nodes (0 .. depth - 2), then the legs: leg j holds
    triangles 2 j (child 0) and 2 j + 1 (child 1); spine node i holds leg i
    and spine node i + 1, the last one legs depth - 2 and depth - 1."""
    assert depth >= 2
    k = depth - 1
    V = _triangles(2 * depth, 200 + depth)
    bvh = np.zeros((k + depth, 4, 4), np.float32)
    leg = lambda j: 4 * (k + j)                                                           # noqa: E731
    for i in range(k):
        last = i + 1 == k
        _node(bvh, i, _box(V[2 * i:2 * i + 2]), leg(i), _box(V[2 * i + 2:]), leg(i + 1) if last else 4 * (i + 1))
    for j in range(depth):
        _node(bvh, k + j, _box(V[2 * j]), ~(8 * j), _box(V[2 * j + 1]), ~(8 * j + 4))
    return _frozen(_flat(bvh, V, 200 + depth))


TIES = ("deepest", "deepest-swapped", "root")


@functools.lru_cache(maxsize=None)
def tie_comb(depth, where):
    """A comb whose nearest triangle (a wide wedge here) occurs twice:
    `deepest`: as both leaves of the deepest node (root-path keys of `depth`
    levels each), child 0 the lower slots; `deepest-swapped`: child 0 the
    higher slots; `root`: as the root's leaf and the deepest leaf.  The two
    copies have opposite normals."""
    assert where in TIES
    V = _triangles(depth + 1, 300 + depth, tie=where)
    V[0 if where == "root" else depth - 1] = V[depth]
    flat = _comb(V, depth, 300 + depth, swap_last=where == "deepest-swapped")
    flat["normals"][4 * depth:4 * depth + 3, :3] *= np.float32(-1.0)
    return _frozen(flat)


def tie_slots(depth, where):
    """(winner, loser): the first slots of the coincident triangles, the
    winner the one the reference's walk tests first."""
    a, b = (0, depth) if where == "root" else (depth - 1, depth)
    return (4 * b, 4 * a) if where == "deepest-swapped" else (4 * a, 4 * b)


def tree(kind, depth):
    return comb_tree(depth) if kind == "comb" else legged_comb_tree(depth)


def render_cases():
    """(kind, depth, cfg) of the renders test_gpu_stack.py compares with the
    oracle: the comb at every depth and the legged comb at three, C2 and C3 at
    every depth, plain HDRI + mesh (C5's flags) and C2D (a class kernel) up to 30."""
    trees = [("comb", d) for d in DEPTHS] + [("legged", d) for d in LEGGED_DEPTHS]
    return [(k, d, cfg) for k, d in trees for cfg in SCENES if cfg in ("C2", "C3") or d <= 30]


def mesh_stack_entries(depth) -> int:
    """mesh_stack_entries of vr_ctx.hpp, read from the header."""
    from vrenderer_pathtracer_amd import build
    with open(os.path.join(build.CSRC, "vr_ctx.hpp")) as f:
        m = re.search(r"^inline int mesh_stack_entries\(uint32_t depth\) \{ return (.*); \}$", f.read(), re.M)
    steps = re.fullmatch(r"depth <= (\d+) \? (\d+) : depth <= (\d+) \? (\d+) : depth <= (\d+) \? (\d+) : (\d+)", m.group(1))
    v = [int(x) for x in steps.groups()]
    return next((n for lim, n in zip(v[0:6:2], v[1:6:2]) if depth <= lim), v[6])


def _frozen(flat):
    for a in flat.values():
        a.setflags(write=False)
    return flat


# ---- scenes -----------------------------------------------------------------------------
SCENES = ("C2", "C3", "C5", "C2D")


def scene(flat, cfg="C2", width=W, height=H) -> dict:
    """The scene of configuration `cfg` (its flags; small maps) around a comb,
    seen by the camera on the axis: every camera ray pierces every leaf box."""
    import flag_lattice as fl
    inp = fl._inputs()
    sc = dict(camera=dict(CAMERA), fresnel_coef=0.1, fresnel_pow=3.0, width=width, height=height, time=TIMES[0],
              cornell=cfg in ("C2", "C2D"), example_sphere=False, view_brdf=False, mesh_flat=flat, name=cfg)
    if not sc["cornell"]:
        sc["hdr"] = inp["hdr"]
    for key in {"C3": ("tex_diffuse", "tex_normal", "tex_specular"), "C2D": ("tex_diffuse",)}.get(cfg, ()):
        sc[key] = inp[key]
    return sc


def view_half_extent(sc, z) -> tuple:
    """Half the view's width and height on the plane at z."""
    cam = sc["camera"]
    dist = cam["origin"][2] - z
    return 0.5 * cam["fov_scale"] * sc["width"] / sc["height"] * dist, 0.5 * cam["fov_scale"] * dist


# ---- rays ---------------------------------------------------------------------------------
RAY_KINDS = ("spine", "side", "spine", "random", "spine", "side", "spine", "spine")    # by i % 8
TMAX_KINDS = ("none",) * 6 + ("below", "between")                                      # as ray_set: by i % 8


def spine_rays(flat, n, seed=20241101) -> dict:
    """n rays, origins, dirs (n,3), tmax (n,), kind (n,) str, interleaved by i % 8:
    `spine`: from a disc of radius 0.5 around the camera, down the axis and
    diverging by at most 0.008: every leaf box is pierced; `side`: aimed at a
    triangle's centroid from 40 away, 80 degrees off the axis: few boxes;
    `random`: as ray_set's.  No direction component is zero.  tmax cycles as
    in ray_set: rays 6 and 7 of every eight have one below the nearest hit
    (a miss) and one between the first and the second hit."""
    rng = np.random.default_rng(seed)
    _, V = flat_triangles(flat)
    cen = V.astype(np.float64).mean(1)
    kind = np.array([RAY_KINDS[i % 8] for i in range(n)])
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        if kind[i] == "spine":
            r, a = 0.5 * np.sqrt(rng.uniform()), rng.uniform(0, 2 * np.pi)
            o[i] = [r * np.cos(a), r * np.sin(a), CAMERA["origin"][2]]
            r, a = rng.uniform(0.0005, 0.008), rng.uniform(0, 2 * np.pi)
            d[i] = np.array([r * np.cos(a), r * np.sin(a), -1.0]) * rng.uniform(0.5, 2.0)
        elif kind[i] == "side":
            a, phi = rng.uniform(0, 2 * np.pi), np.deg2rad(80.0)
            away = np.array([np.sin(phi) * np.cos(a), np.sin(phi) * np.sin(a), np.cos(phi)])
            c = cen[int(rng.integers(0, len(cen)))]
            o[i] = c + 40.0 * away
            d[i] = c - np.float32(o[i]).astype(np.float64)
        else:
            o[i] = rng.uniform(-40.0, 40.0, 3)
            d[i] = rng.normal(0, 1, 3)
    o, d = o.astype(np.float32), d.astype(np.float32)
    assert (d != 0).all()
    tmax = np.full(n, NO_HIT, np.float32)
    acc, dist, _, _ = brute_force(V, o, d)
    for i in range(n):
        ts = np.unique(dist[i][acc[i]])
        if TMAX_KINDS[i % 8] == "none" or len(ts) == 0:
            continue
        if TMAX_KINDS[i % 8] == "below":
            tmax[i] = ts[0] * F(0.5)
        else:
            tmax[i] = (ts[0] + ts[1]) * F(0.5) if len(ts) > 1 and (ts[0] + ts[1]) * F(0.5) > ts[0] else ts[0] * F(2.0)
    out = dict(origins=o, dirs=d, tmax=tmax, kind=kind)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rays_of(kind, depth, n):
    return spine_rays(tree(kind, depth), n)


# ---- the reference walk's high-water mark -----------------------------------------------------
def high_water(flat, o, d) -> int:
    """The largest stack pointer of the reference's walk (oracle/vro.c
    intersect_scene, PathTracer.cu:269-464) for one ray: its push and pop rule
    restated on ray_query_cases' fp32 slab arithmetic.  No triangle is tested:
    the reference's walk does not shorten the ray, so which boxes it enters
    does not depend on the hits."""
    bvh = np.asarray(flat["bvh"], np.float32).reshape(-1, 4, 4)
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        inv = np.array([F(1.0) / (d[a] if abs(d[a]) > EPS else EPS) for a in range(3)], np.float32)
    sentinel = 0x76543210
    stack, sp, top = {0: sentinel}, 0, 0
    leaf, node = 0, 0
    while node != sentinel:
        while 0 <= node < sentinel:
            n = bvh[node // 4]
            idx0, idx1 = (int(x) for x in n[3, :2].copy().view(np.int32))
            with np.errstate(all="ignore"):
                (c0min, c0max), (c1min, c1max) = _span(n, 0, o, inv), _span(n, 1, o, inv)
            swp, tc0, tc1 = c1min < c0min, c0max >= c0min, c1max >= c1min
            if not tc0 and not tc1:
                node, sp = stack[sp], sp - 1
            else:
                node = idx0 if tc0 else idx1
                if tc0 and tc1:
                    if swp:
                        node, idx1 = idx1, node
                    sp += 1
                    stack[sp] = idx1
                    top = max(top, sp)
            if node < 0 and leaf >= 0:
                leaf = node
                node, sp = stack[sp], sp - 1
            if not leaf >= 0:
                break
        while leaf < 0:
            leaf = node
            if node < 0:
                node, sp = stack[sp], sp - 1
    return top


# ---- the oracle with a stack of a settable size --------------------------------------------------
def build_driver() -> str:
    import surface_cases as sf
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
    L.stack_driver_capacity.restype = ctypes.c_int
    L.stack_driver_capacity.argtypes = [ctypes.c_int]
    L.stack_driver_rays.restype = ctypes.c_int
    L.stack_driver_rays.argtypes = [ctypes.POINTER(po.VroScene), vp, vp, ctypes.c_uint32, vp, vp, vp, vp]
    L.vro_render.restype = ctypes.c_int
    L.vro_render.argtypes = po.lib().vro_render.argtypes
    return L


def driver_render(sc, capacity, frames, times=TIMES):
    """(accum, rgba8, depth8, max_stack) of the portable-libm oracle with a
    stack of `capacity` entries that loses the pushes it cannot hold."""
    L = driver()
    assert L.stack_driver_capacity(int(capacity)) == 0
    osc = po.OracleScene(sc, libm=po.LIBM_PORTABLE)
    accum = np.zeros((osc.height, osc.width, 4), np.float32)
    rgba, depth = (np.zeros((osc.height, osc.width, 4), np.uint8) for _ in range(2))
    t = (ctypes.c_uint32 * frames)(*[int(v) & 0xFFFFFFFF for v in times[:frames]])
    cnt = po.VroCounters()
    err = L.vro_render(ctypes.byref(osc.s), po._fp(accum), rgba.ctypes.data, depth.ctypes.data, 1, frames, t, 0, osc.height,
                       0, ctypes.byref(cnt))
    assert err == 0, err
    return accum, rgba, depth, int(cnt.max_stack)


def driver_rays(sc, origins, dirs, capacity):
    """(records [n, 26] uint32, high_water [n]): intersect_scene's hit flag,
    hit type and the six rows of its hit_t for every ray, the directions
    normalised as surface_cases.normalised does, with a stack of `capacity` entries; and each ray's largest stack pointer."""
    L = driver()
    assert L.stack_driver_capacity(int(capacity)) == 0
    osc = po.OracleScene(sc, libm=po.LIBM_PORTABLE)
    o, d = np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(dirs, np.float32)
    n = len(o)
    rows = np.zeros((n, 24), np.float32)
    types, top = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    hit = np.zeros(n, np.int32)
    err = L.stack_driver_rays(ctypes.byref(osc.s), o.ctypes.data, d.ctypes.data, n, rows.ctypes.data, types.ctypes.data,
                              hit.ctypes.data, top.ctypes.data)
    assert err == 0, err
    return np.concatenate([hit.view(np.uint32)[:, None], types[:, None], rows.view(np.uint32)], 1), top.astype(np.int64)


def query_cases():
    """(kind, depth, cfg) of the query tests: every tree of the render cases, in C2 and in C3."""
    return [(k, d, cfg) for k, d, cfg in render_cases() if cfg in ("C2", "C3")]


@functools.lru_cache(maxsize=None)
def query_case(kind, depth, cfg):
    """What the radiance, surface and shade queries must return on the
    tree's spine rays, by the yardsticks of radiance_cases, surface_cases and
    shade_cases: dict scene, origins, dirs, seeds, paths [n, 2, 4] (the
    oracle's trace), records [n, 28] (its intersect_scene), shaded [n, 2, 4]
    (shade_driver.c on those records) and kept [n] (every float finite in all
    three).  Computed once, never written."""
    import radiance_cases as rc
    import shade_cases as sh
    import surface_cases as sf
    rays = rays_of(kind, depth, N_QUERY)
    sc = scene(tree(kind, depth), cfg)
    o, d = rays["origins"], rays["dirs"]
    s = np.random.default_rng(20241102).integers(0, 2**32, (N_QUERY, 2), dtype=np.uint64).astype(np.uint32)
    paths = rc.oracle_paths(sc, o, d, s, 2)
    records = sf.yardstick(sc, o, d)
    shaded = sh.driver_paths(sc, records, d, s, 2)
    kept = np.isfinite(paths).all((1, 2)) & sf.finite(records) & np.isfinite(shaded).all((1, 2))
    assert (~kept).sum() <= rc.MAX_DROPPED * N_QUERY, f"{(~kept).sum()} of {N_QUERY} rays are not finite under a yardstick"
    out = dict(scene=sc, origins=o, dirs=d, seeds=s, paths=paths, records=records, shaded=shaded, kept=kept)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def oracle_render(sc, frames, times=TIMES, count=False):
    """The portable-libm oracle's (accum, rgba8, depth8, counters), never written."""
    out = po.render(sc, frames=frames, times=list(times[:frames]), libm=po.LIBM_PORTABLE, count=count)
    for a in out[:3]:
        a.setflags(write=False)
    return out
