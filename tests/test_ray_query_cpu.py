"""The host ray query (vrhip_flat_trace_rays, vr_raycast.cpp), the yardstick
of the device query: against a numpy brute force of the reference's triangle
test, which is itself checked against the oracle's intersectTriangle; the
winner of exact ties against an independent depth-first ordering; any-hit;
refusals and non-finite rays.  Every comparison is bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

from device_mesh_cases import hard_mesh, soup
from ray_query_cases import (NO_HIT, brute_force, chain_tree, closest, dfs_slots, flat_triangles, ray_set, same_bits,
                             tri_test, u32)
from vrenderer_pathtracer_amd import VRHIPError, build_flat, flat_trace_rays

N_RAYS = 1000


@functools.lru_cache(maxsize=None)
def soup_case(n, leaf):
    flat = build_flat(soup(n), leaf)
    slots, V = flat_triangles(flat)
    rays = ray_set(V, N_RAYS)
    return flat, slots, V, rays, brute_force(V, rays["origins"], rays["dirs"], rays["tmax"])


def check_against_brute_force(flat, slots, V, rays, bf, got):
    acc, dist, u, v = bf
    hit, tmin = closest(acc, dist)
    assert (got["prim"] >= 0).tolist() == hit.tolist()
    assert same_bits(got["t"][hit], tmin[hit])
    assert same_bits(got["t"][~hit], rays["tmax"][~hit])                # a miss reports its tmax
    assert not u32(got["u"][~hit]).any() and not u32(got["v"][~hit]).any()
    col = np.searchsorted(slots, got["prim"][hit])
    assert (slots[col] == got["prim"][hit]).all()                        # a triangle's first slot
    rows = np.flatnonzero(hit)
    assert acc[rows, col].all() and same_bits(dist[rows, col], tmin[hit])   # one of the closest triangles
    assert same_bits(got["u"][hit], u[rows, col]) and same_bits(got["v"][hit], v[rows, col])
    return hit


# ---- 1. the host walk against brute force -------------------------------------------
@pytest.mark.parametrize("leaf", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 65, 1000])
def test_host_walk_equals_brute_force(native, n, leaf):
    flat, slots, V, rays, bf = soup_case(n, leaf)
    got = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"])
    hit = check_against_brute_force(flat, slots, V, rays, bf, got)
    kind = rays["kind"]
    assert hit[np.isin(kind, ["aim", "half", "triple"])].all()          # aimed at a centroid: certain hits
    assert not hit[kind == "below"].any()                               # tmax below the nearest hit
    assert hit[kind == "between"].all()                                 # tmax behind the first hit only
    if n >= 65:
        assert 0 < hit[kind == "random"].sum() < (kind == "random").sum()
    # directions are used as given: the centroid lies at t = 1 / scale along them
    for k, s in (("aim", 1.0), ("half", 0.5), ("triple", 3.0)):
        assert (got["t"][kind == k] < 1.001 / s).all()


def test_brute_force_equals_the_oracle_triangle_test(native, oracle):
    """All four outputs of vro_intersect_triangle, on every ray's winning
    triangle and on 2000 random (ray, triangle) pairs."""
    L = oracle.lib()
    flat, slots, V, rays, (acc, dist, u, v) = soup_case(1000, 3)
    hit, tmin = closest(acc, dist)
    win = np.where(acc & (u32(dist) == u32(tmin)[:, None]), np.arange(len(slots))[None, :], len(slots)).min(1)
    rng = np.random.default_rng(8)
    pairs = [(int(i), int(win[i])) for i in np.flatnonzero(hit)]
    pairs += list(zip(rng.integers(0, N_RAYS, 2000).tolist(), rng.integers(0, len(slots), 2000).tolist()))
    f4 = lambda a: (ctypes.c_float * 4)(*[float(x) for x in a], 0.0)     # noqa: E731
    out = (ctypes.c_float * 4)()
    n_hits = 0
    for i, t in pairs:
        L.vro_intersect_triangle(f4(V[t, 0]), f4(V[t, 1]), f4(V[t, 2]), f4(rays["origins"][i]), f4(rays["dirs"][i]), out)
        ok, bd, bu, bv = tri_test(V[t, 0], V[t, 1], V[t, 2], rays["origins"][i], rays["dirs"][i])
        want = np.array([bd, bu, bv, 0.0], np.float32) if ok else np.zeros(4, np.float32)
        assert same_bits(np.array(list(out), np.float32), want), (i, t, list(out), want)
        n_hits += bool(ok)
    assert n_hits >= hit.sum() > 500


# ---- 3. ties ----------------------------------------------------------------------------
def check_ties(flat, o, d, min_ties):
    """The host walk against a second ordering computed here: the triangles of
    the leaves whose boxes the ray's line pierces, depth first and near child
    first (dfs_slots, a recursive walk with float min / max), the brute-force
    test on each, the first of the closest.  A ray that grazes a box -- one
    aimed exactly at a mesh vertex does -- can miss it in fp32 and with it a
    triangle the brute force over all triangles accepts; the reference's walk
    has that property, so the expectation is taken over the pierced leaves.
    Returns, per ray, how many triangles tie at the closest distance."""
    slots, V = flat_triangles(flat)
    col_of = {int(s): c for c, s in enumerate(slots)}
    acc, dist, u, v = brute_force(V, o, d)
    got = flat_trace_rays(flat, o, d)
    tied = np.zeros(len(o), np.int64)
    for i in range(len(o)):
        cols = [col_of[s] for s in dfs_slots(flat, o[i], d[i])]
        cols = [c for c in cols if acc[i, c]]
        if not cols:
            assert got["prim"][i] == -1, (i, got["prim"][i])
            continue
        tmin = min(dist[i, c] for c in cols)
        winners = [c for c in cols if dist[i, c] == tmin]
        tied[i] = len(winners)
        assert got["prim"][i] == slots[winners[0]], (i, got["prim"][i], [int(slots[c]) for c in winners])
        assert same_bits(got["t"][i], tmin)
        assert same_bits(got["u"][i], u[i, winners[0]]) and same_bits(got["v"][i], v[i, winners[0]])
    assert (tied > 1).sum() >= min_ties, (tied > 1).sum()
    return tied


def test_ties_on_coincident_triangles(native):
    """Every hit is a 50-way tie: the winner is the first triangle of the flat
    tree in depth-first, near-child-first order."""
    m = hard_mesh("identical")
    for leaf in (1, 2, 3):
        flat = build_flat(m, leaf)
        slots, V = flat_triangles(flat)
        rays = ray_set(V, 96)
        tied = check_ties(flat, rays["origins"], rays["dirs"], min_ties=30)
        assert set(tied[tied > 0].tolist()) == {50}


def test_ties_on_shared_vertices_and_edges(native):
    m = hard_mesh("shared")
    flat = build_flat(m, 2)
    P, tris = m["positions"], m["tris"].astype(np.int64)
    rng = np.random.default_rng(3)
    pick = rng.choice(len(tris), 60, replace=False)
    targets = np.concatenate([P[tris[pick, 0]],                                            # mesh vertices
                              (P[tris[pick, 0]] + P[tris[pick, 1]]) * np.float32(0.5)])    # edge midpoints
    side = rng.normal(0, 1, (len(targets), 3))
    o = (side / np.linalg.norm(side, axis=1, keepdims=True) * 200.0).astype(np.float32)
    d = (targets - o).astype(np.float32)
    check_ties(flat, o, d, min_ties=0)
    # the exact case: an origin on the vertex's own axis-aligned line hits it at an exactly representable point
    o2 = targets.copy()
    o2[:, 2] += np.float32(256.0)
    d2 = np.zeros_like(o2)
    d2[:, 2] = -1.0
    check_ties(flat, o2, d2, min_ties=1)


# ---- 4. any-hit ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,leaf", [(1, 1), (5, 3), (65, 1), (1000, 3)])
def test_any_hit_equals_closest_hit(native, n, leaf):
    flat, slots, V, rays, bf = soup_case(n, leaf)
    hit = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"])["prim"] >= 0
    got = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"], any_hit=True)
    assert (got["prim"] >= 0).tolist() == hit.tolist()
    for k in ("t", "u", "v"):
        assert not u32(got[k][hit]).any()
    assert not got["prim"][hit].any()
    assert same_bits(got["t"][~hit], rays["tmax"][~hit])


# ---- a deep tree ---------------------------------------------------------------------------------
def test_chain_tree(native):
    flat = chain_tree(40)
    slots, V = flat_triangles(flat)
    rays = ray_set(V, 256)
    bf = brute_force(V, rays["origins"], rays["dirs"], rays["tmax"])
    got = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"])
    hit = check_against_brute_force(flat, slots, V, rays, bf, got)
    assert hit.sum() > 64


# ---- 5. refusals and non-finite rays -----------------------------------------------------------
def test_refusals(native):
    L = native
    flat, slots, V, rays, _ = soup_case(5, 3)
    bvh, verts = np.ascontiguousarray(flat["bvh"]), np.ascontiguousarray(flat["verts"])
    o, d = rays["origins"][:4].copy(), rays["dirs"][:4].copy()
    rec = np.zeros((4, 4), np.int32)
    fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))   # noqa: E731
    hp = ctypes.c_void_p(rec.ctypes.data)

    def call(bvh=bvh, verts=verts, o=o, d=d, n=4, mode=0, hits=hp, n_bvh=None):
        return L.vrhip_flat_trace_rays(fp(bvh), bvh.size // 4 if n_bvh is None else n_bvh, fp(verts),
                                       0 if verts is None else verts.size // 4, fp(o), fp(d), None, n, mode, hits)
    assert call() == 0
    assert call(o=None) == -1 and call(d=None) == -1 and call(hits=None) == -1 and call(verts=None) == -1
    assert call(mode=2) == -1
    assert call(n=0, o=None, d=None, hits=None) == 0                 # nothing to write
    cyc = bvh.copy()
    cyc.view(np.int32)[3, 0] = 0                                     # the root's child 0 is the root
    assert call(bvh=cyc) == -4
    far = bvh.copy()
    far.view(np.int32)[3, 1] = 4 * 1000                              # a child offset out of range
    assert call(bvh=far) == -4
    open_run = verts.copy()
    open_run[u32(verts[:, 0]) == 0x80000000, 0] = 1.0                # no terminator anywhere
    assert call(verts=open_run) == -4
    assert call(n_bvh=bvh.size // 4 - 1) == -4
    with pytest.raises(VRHIPError):
        flat_trace_rays(dict(bvh=cyc, verts=verts), o, d)
    # the device call refuses a null context without a device
    assert L.vrhip_trace_rays(None, None, None, None, 0, 0, None) == -1
    assert L.vrhip_trace_rays(None, hp, hp, None, 4, 0, hp) == -1


def test_non_finite_rays_are_misses(native):
    flat, slots, V, rays, _ = soup_case(65, 1)
    aimed = np.flatnonzero(rays["kind"] == "aim")[:8]
    o, d = rays["origins"][aimed].copy(), rays["dirs"][aimed].copy()
    tmax = np.full(8, 50.0, np.float32)
    o[0, 1] = np.nan
    d[1, 2] = np.inf
    o[2, 0] = -np.inf
    d[3] = np.nan
    tmax[4] = np.nan
    tmax[5] = np.inf                                                 # a bound like any other
    for any_hit in (False, True):
        got = flat_trace_rays(flat, o, d, tmax, any_hit=any_hit)
        assert got["prim"][:5].tolist() == [-1] * 5
        assert same_bits(got["t"][:5], np.full(5, NO_HIT, np.float32))
        assert not u32(got["u"][:5]).any() and not u32(got["v"][:5]).any()
        assert (got["prim"][5:] >= 0).all()
    clean = flat_trace_rays(flat, rays["origins"][aimed][6:], rays["dirs"][aimed][6:], tmax[6:])
    got = flat_trace_rays(flat, o, d, tmax)
    assert all(same_bits(got[k][6:], clean[k]) for k in ("t", "u", "v")) and (got["prim"][6:] == clean["prim"]).all()
