"""Geometry and rays at the extremes of float, shared by test_extreme_cpu.py and
test_gpu_extreme.py (and, for the tree checks, test_gpu_device_sah.py and
test_gpu_refit.py): the meshes of EXTREME_KINDS, the extreme ray set, two
constructions whose slab arithmetic is NaN, the numpy expectation of the
reference walk over the leaves it pierces, the NaN-aware record comparison
and the exact-box check of a flattened tree.

EXTREME_KINDS is not part of device_mesh_cases.HARD_KINDS: that list feeds the
recorded digests (tests/golden/devmesh_digests.json)."""
import numpy as np

from device_mesh_cases import expected_triangles, sorted_rows, soup
from ray_query_cases import NO_HIT, brute_force, dfs_slots, flat_triangles, u32
from vrenderer_pathtracer_amd import validate_flat

TERM = 0x80000000
MAX_BUILD_DEPTH = 30                                   # kMaxBuildDepth
FLT_MAX = np.float32(3.4028234663852886e38)
N_TRIS = 200

EXTREME_KINDS = ["big", "huge", "wide", "tiny"]
# The seed of `wide`: the first one, counting from 1, whose host tree stays
# inside the depth cap with leaves of 1 and of 3 triangles
# (test_extreme_cpu.test_wide_builds_next_to_the_depth_cap asserts it).
WIDE_SEED = 1


# ---- meshes -------------------------------------------------------------------
def extreme_mesh(kind):
    """A seeded soup of 200 triangles, every value finite.  big: products of
    two coordinates near overflow.  huge: the extent hi - lo and the centroids
    0.5f * (lo + hi) overflow.  wide: triangle sizes over 60 decades, a tree
    about as deep as the builder allows.  tiny: denormal coordinates and edges."""
    m = soup(N_TRIS)
    P = m["positions"].astype(np.float64)
    if kind == "big":
        P = P * 1e18
    elif kind == "huge":
        P = np.clip(P * 1e37, -3.4e38, 3.4e38)
    elif kind == "wide":
        rng = np.random.default_rng(WIDE_SEED)
        P = (P.reshape(N_TRIS, 3, 3) * 10.0 ** rng.uniform(-30, 30, (N_TRIS, 1, 1))).reshape(-1, 3)
    elif kind == "tiny":
        P = P * 1e-40
    else:
        raise ValueError(kind)
    m["positions"] = P.astype(np.float32)
    assert np.isfinite(m["positions"]).all()
    return m


def offset_mesh(offset):
    """A small soup (80 triangles, extent about 12) moved by `offset` along every
    axis: at 1e3 its coordinates are 80 times its extent, at 1e6 they pass the
    largest half and one float ulp is a twentieth of a triangle."""
    m = soup(80, seed=7, spread=5.0, sigma=1.0)
    m["positions"] = (m["positions"].astype(np.float64) + offset).astype(np.float32)
    return m


def depth_cap_mesh(n_peel=29, n_cluster=130, ratio=300.0):
    """A finite mesh whose SAH tree ends in a leaf of n_cluster >= 128 triangles
    at the depth cap, which the device layout cannot hold: n_peel triangles at
    1e38 * ratio^-i, each alone in the last of the 128 bins of its level, and a
    cluster of distinct denormal triangles that never leaves bin 0."""
    T = n_peel + n_cluster
    P = np.zeros((T, 3, 3))
    base = np.array([[1.0, 1.0, 1.0], [1.1, 1.0, 1.05], [1.0, 1.1, 1.05]])
    for i in range(n_peel):
        P[i] = base * 1e38 * ratio ** -i
    for k in range(n_cluster):
        P[n_peel + k] = np.array([[3 * k, 0, 1], [3 * k + 1, 2, 0], [3 * k + 2, 0, 3]]) * 1.4e-45
    P = P.reshape(-1, 3).astype(np.float32)
    assert np.isfinite(P).all() and len(np.unique(P, axis=0)) == len(P)
    return dict(positions=P, tris=np.arange(3 * T, dtype=np.uint32).reshape(-1, 3))


# ---- rays ------------------------------------------------------------------------
LADDER = [1e-45, 1e-38, 1e-30, 1e-10, 1.0, 1e10, 1e19, 1e30, 3e38]
TMAX_CYCLE = [1e20, np.inf, 0.0, -1.0, 1e-30, 3e38, 1.0, -np.inf]
# 11 slots against 8 tmax values: every pair occurs.  Aimed rays take 7 of the 11: only they can hit
DIR_KINDS = ["aim", "random", "aim", "axis", "aim", "aim", "zero", "aim", "negzero", "aim", "aim"]


def _f32(a):
    with np.errstate(over="ignore"):
        return np.clip(np.asarray(a, np.float64), -float(FLT_MAX), float(FLT_MAX)).astype(np.float32)


def extreme_ray_set(V, n, seed=20241020):
    """n finite rays against the triangles V (T,3,3).  The magnitude of the
    origin (its distance from the mesh's middle) and of the direction are
    drawn independently from LADDER.  Directions: 'aim' (at a centroid, then
    scaled to the drawn magnitude and clipped to finite), 'random', 'axis' (one
    component, exact zeros elsewhere), 'zero' (all three zero) and 'negzero'
    (zero with one -0).  tmax cycles through TMAX_CYCLE.
    Returns dict origins, dirs (n,3), tmax (n,), kind (n,) str."""
    rng = np.random.default_rng(seed)
    T = len(V)
    mid = (V.reshape(-1, 3).min(0).astype(np.float64) + V.reshape(-1, 3).max(0)) / 2
    cen = (V[:, 0].astype(np.float64) + V[:, 1] + V[:, 2]) / 3.0
    kind = np.array([DIR_KINDS[i % len(DIR_KINDS)] for i in range(n)])
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        omag, dmag = LADDER[int(rng.integers(len(LADDER)))], LADDER[int(rng.integers(len(LADDER)))]
        tri = int(rng.integers(0, T))
        side = rng.normal(0, 1, 3)
        side /= np.linalg.norm(side)
        o[i] = _f32(mid + side * omag)
        if kind[i] == "aim":
            to = cen[tri] - o[i]
            norm = np.linalg.norm(to / np.abs(to).max()) * np.abs(to).max()
            d[i] = to / norm * dmag if norm > 0 else side * dmag
        elif kind[i] == "random":
            w = rng.normal(0, 1, 3)
            d[i] = w / np.linalg.norm(w) * dmag
        elif kind[i] == "axis":
            ax, sign = int(rng.integers(0, 3)), rng.choice([-1.0, 1.0])
            o[i] = np.float32(cen[tri])
            o[i, ax] = _f32(cen[tri][ax] - sign * omag)
            d[i, ax] = sign * dmag
        elif kind[i] == "negzero":
            d[i, int(rng.integers(0, 3))] = -0.0
    tmax = np.array([TMAX_CYCLE[i % len(TMAX_CYCLE)] for i in range(n)], np.float32)
    o, d = _f32(o), _f32(d)
    assert np.isfinite(o).all() and np.isfinite(d).all()
    return dict(origins=o, dirs=d, tmax=tmax, kind=kind)


def near_ray_set(V, n, seed=77):
    """n rays aimed at centroids of the triangles V, unit directions scaled by
    0.5 .. 2, tmax 1e20 or +inf.  Even rays start 2 to 20 times the mesh's half
    diagonal from its middle: across the distance at which the query kernel
    stops trusting the culled walk (8 extents).  Odd rays start 2 to 10 times
    the mesh's largest |coordinate| from its middle: the same family on a
    centred mesh, millions of extents out on a small mesh far from zero, where
    a rule that measured distance against coordinates would keep them."""
    rng = np.random.default_rng(seed)
    P = V.reshape(-1, 3).astype(np.float64)
    mid, half = (P.min(0) + P.max(0)) / 2, np.linalg.norm(P.max(0) - P.min(0)) / 2
    big = np.abs(P).max()
    cen = V.astype(np.float64).mean(1)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        side = rng.normal(0, 1, 3)
        away = big * rng.uniform(2, 10) if i % 2 else half * rng.uniform(2, 20)
        o[i] = np.float32(mid + side / np.linalg.norm(side) * away)
        to = cen[int(rng.integers(len(V)))] - o[i]
        d[i] = to / np.linalg.norm(to) * rng.uniform(0.5, 2)
    tmax = np.array([TMAX_CYCLE[i % 2] for i in range(n)], np.float32)
    return dict(origins=o.astype(np.float32), dirs=d.astype(np.float32), tmax=tmax, kind=np.array(["near"] * n))


def nan_plane_case(both, n=96, seed=9):
    """(mesh, rays): slab arithmetic that is NaN by construction.  The rays
    travel in a plane z = const (direction z exactly 0, so the walk divides
    by the 3e-10 replacement, 1 / 3e-10 = 3.3e9) towards a point of a triangle
    from an origin at that point's height.  The triangles are 1e29 tall along
    z and ordinary along x and y, so every product of the triangle test stays
    finite and the brute force hits.
    both=True: every z of the mesh, and the origin's, is at least 1e30:
      n * inv and o * inv overflow with the same sign, and both planes of
      every box are inf - inf.
    both=False: every triangle aimed at straddles z = 0, and so does every box
      above it, and the origin's z is positive: the low plane is
      -inf - inf = -inf, the high one inf - inf, and the integer comparison of
      the reference's span reads the sign of that NaN: set, as the device
      makes it, and the box is missed; clear, and z would drop out of the span
      and every one of these rays would hit."""
    m = soup(N_TRIS)
    rng = np.random.default_rng(seed)
    P = m["positions"].astype(np.float64)
    P[:, 2] = P[:, 2] * 1e29 + 1e31 if both else rng.normal(0, 10, len(P)) * 1e29
    m["positions"] = P.astype(np.float32)
    V = m["positions"][m["tris"].astype(np.int64)].astype(np.float64)
    top = np.argmax(V[..., 2], 1)
    w = np.full((len(V), 3), 0.25)
    w[np.arange(len(V)), top] = 0.5
    target = (w[..., None] * V).sum(1)                     # inside the triangle, towards its highest vertex
    if both:
        assert (V[..., 2] >= 1e30).all()
        pick = np.arange(len(V))
    else:
        pick = np.flatnonzero((V[..., 2].min(1) < 0) & (target[:, 2] >= 2e29))
        assert len(pick) >= 50
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        c = target[pick[int(rng.integers(len(pick)))]]
        a = rng.uniform(0, 2 * np.pi)
        o[i] = [c[0] + 100 * np.cos(a), c[1] + 100 * np.sin(a), c[2]]
        d[i] = [c[0] - o[i, 0], c[1] - o[i, 1], -0.0 if i % 2 else 0.0]
    o, d = o.astype(np.float32), d.astype(np.float32)
    assert (o[:, 2] >= 2e29).all() and (d[:, 2] == 0).all()
    tmax = np.array([TMAX_CYCLE[i % 2] for i in range(n)], np.float32)            # 1e20 and +inf
    return m, dict(origins=o, dirs=d, tmax=tmax, kind=np.array(["plane"] * n))


# ---- the expectation: the reference walk over the leaves it pierces --------------------
def walk_expectation(flat, rays, use_tmax=True):
    """Per ray the record of the reference's closest-hit walk, from pieces that
    share no code with it: the triangles of the leaves whose boxes the ray's
    line pierces, depth first and near child first (ray_query_cases.dfs_slots),
    the numpy triangle test on each, the first of the closest.  Also returns
    the brute force's verdict over all triangles: at the extremes the slab
    arithmetic overflows and the walk misses triangles the brute force
    accepts, as the reference's does.
    Returns (dict t, prim, u, v, hit), brute_hit (N,) bool."""
    slots, V = flat_triangles(flat)
    col_of = {int(s): c for c, s in enumerate(slots)}
    o, d = rays["origins"], rays["dirs"]
    t0 = rays["tmax"] if use_tmax else np.full(len(o), NO_HIT, np.float32)
    acc, dist, u, v = brute_force(V, o, d, t0)
    n = len(o)
    want = dict(t=t0.astype(np.float32).copy(), prim=np.full(n, -1, np.int64), u=np.zeros(n, np.float32),
                v=np.zeros(n, np.float32))
    for i in range(n):
        if not acc[i].any():                               # no triangle can be accepted: the order is moot
            continue
        cols = [col_of[s] for s in dfs_slots(flat, o[i], d[i])]
        cols = [c for c in cols if acc[i, c]]
        if not cols:
            continue
        tmin = min(dist[i, c] for c in cols)
        win = next(c for c in cols if dist[i, c] == tmin)
        want["t"][i], want["prim"][i], want["u"][i], want["v"][i] = tmin, slots[win], u[i, win], v[i, win]
    want["hit"] = want["prim"] >= 0
    return want, acc.any(1)


# ---- comparing records ----------------------------------------------------------------------
def same_float_nan_aware(a, b):
    """Bit for bit, except that a NaN equals any NaN (its sign and payload are
    unspecified: vrhip.h, vrhip_trace_rays)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (u32(a) == u32(b)) | (np.isnan(a) & np.isnan(b))


def assert_same_records(a, b, what, prim=True):
    """t by bits and never NaN; u, v by bits or both NaN; hit or miss; prim
    (only where both sides name triangles the same way)."""
    assert not np.isnan(a["t"]).any() and not np.isnan(b["t"]).any(), what
    bad = np.flatnonzero(u32(a["t"]) != u32(b["t"]))
    assert len(bad) == 0, f"{what}: t differs on {len(bad)} rays (first {bad[:5].tolist()})"
    for k in ("u", "v"):
        bad = np.flatnonzero(~same_float_nan_aware(a[k], b[k]))
        assert len(bad) == 0, f"{what}: {k} differs on {len(bad)} rays (first {bad[:5].tolist()})"
    ha, hb = np.asarray(a["prim"]) >= 0, np.asarray(b["prim"]) >= 0
    assert (ha == hb).all(), what
    if prim:
        bad = np.flatnonzero(np.asarray(a["prim"], np.int64) != np.asarray(b["prim"], np.int64))
        assert len(bad) == 0, f"{what}: prim differs on {len(bad)} rays (first {bad[:5].tolist()})"


# ---- the exported tree -------------------------------------------------------------------------
def slot_rows(flat):
    """(is_term, rows): per non-terminator slot triple, the row expected_triangles gives."""
    verts = flat["verts"]
    is_term = verts[:, 0].copy().view(np.uint32) == TERM
    keep = ~is_term
    assert (verts[keep, 3] == 0).all()
    rows = np.concatenate([verts[keep, :3], flat["normals"][keep, :3], flat["tangents"][keep, :3], flat["uvs"][keep]], -1)
    return is_term, np.ascontiguousarray(rows.reshape(-1, 33))


def check_boxes_and_leaves(flat, mesh, max_leaf):
    """A valid tree with exact boxes (bottom-up, as test_gpu_device_build.analyse),
    every input triangle once, leaves within max_leaf unless the depth cap made them."""
    n_tris = len(mesh["tris"])
    n_refs = max(n_tris, 2)
    depth, n_nodes = validate_flat(flat)
    assert depth <= MAX_BUILD_DEPTH
    nodes = flat["bvh"].reshape(-1, 4, 4)
    assert len(nodes) == n_nodes
    child = nodes[:, 3, :2].copy().view(np.int32)
    verts = flat["verts"]
    is_term, rows = slot_rows(flat)
    term_pos = np.flatnonzero(is_term)
    L = n_nodes + 1
    starts = np.sort(~child[child < 0])
    assert len(starts) == L and len(np.unique(starts)) == L
    ends = term_pos[np.searchsorted(term_pos, starts)]
    counts = (ends - starts) // 3
    assert ((ends - starts) % 3 == 0).all() and counts.min() >= 1
    leaf_level = np.zeros(L, np.int64)                 # the root is level 0
    level, cur = 0, np.array([0])
    while len(cur):
        c = child[cur]
        leaf_level[np.searchsorted(starts, ~c[c < 0])] = level + 1
        level, cur = level + 1, c[c >= 0] // 4
    # only a node the depth cap made a leaf (level kMaxBuildDepth - 1) may hold more than max_leaf
    assert (leaf_level[counts > max_leaf] == MAX_BUILD_DEPTH - 1).all(), counts.max()
    assert starts[0] == 0 and (starts[1:] == ends[:-1] + 1).all() and ends[-1] == len(verts) - 1
    assert len(verts) == 3 * n_refs + L
    want = expected_triangles(mesh)                    # one triangle is stored twice: two rows
    assert np.array_equal(sorted_rows(rows), sorted_rows(want))
    lo_src = np.where(is_term[:, None], np.inf, verts[:, :3]).astype(np.float32)
    hi_src = np.where(is_term[:, None], -np.inf, verts[:, :3]).astype(np.float32)
    leaf_lo = np.minimum.reduceat(lo_src, starts, axis=0)
    leaf_hi = np.maximum.reduceat(hi_src, starts, axis=0)
    levels, cur = [], np.array([0])
    while len(cur):
        levels.append(cur)
        c = child[cur]
        cur = c[c >= 0] // 4
    assert len(levels) == depth
    own_lo = np.zeros((n_nodes, 3), np.float32)
    own_hi = np.zeros((n_nodes, 3), np.float32)
    for lev in reversed(levels):
        los, his = [], []
        for ch in range(2):
            c = child[lev, ch]
            leaf = c < 0
            li = np.searchsorted(starts, np.where(leaf, ~c, 0))
            ni = np.where(leaf, 0, c // 4)
            lo = np.where(leaf[:, None], leaf_lo[li], own_lo[ni])
            hi = np.where(leaf[:, None], leaf_hi[li], own_hi[ni])
            n = nodes[lev]
            stored_lo = np.stack([n[:, ch, 0], n[:, ch, 2], n[:, 2, 2 * ch]], -1)
            stored_hi = np.stack([n[:, ch, 1], n[:, ch, 3], n[:, 2, 2 * ch + 1]], -1)
            assert np.array_equal(stored_lo, lo) and np.array_equal(stored_hi, hi)
            los.append(lo)
            his.append(hi)
        own_lo[lev] = np.minimum(los[0], los[1])
        own_hi[lev] = np.maximum(his[0], his[1])
    return depth, n_nodes
