"""What the ray-query tests share (test_ray_query_cpu.py, test_gpu_ray_query.py):
the triangles of a flattened tree, the fixed ray set, a numpy brute force of
the reference's triangle test, an independent depth-first ordering of a flat
tree, and a hand-made chain tree.  Every float operation of the brute force is
one float32 numpy operation, spelt out componentwise in the C order."""
import numpy as np

TERM = 0x80000000
EPS = np.float32(0.0000000003)
NO_HIT = np.float32(1e20)
SEED = 20240607
F = np.float32


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return bool((u32(a) == u32(b)).all())


# ---- the triangles of a flat tree ------------------------------------------------
def flat_triangles(flat):
    """(slots, V): the slot of every triangle's first vertex and its vertices
    (T,3,3), scanning the leaf runs of flat["verts"] (terminators skipped)."""
    x = u32(flat["verts"][:, 0])
    slots, s = [], 0
    while s < len(x):
        if x[s] == TERM:
            s += 1
        else:
            slots.append(s)
            s += 3
    slots = np.asarray(slots, np.int64)
    V = np.stack([flat["verts"][slots + k, :3] for k in range(3)], 1).astype(np.float32)
    return slots, V


# ---- brute force --------------------------------------------------------------------
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def tri_test(v0, v1, v2, o, d):
    """intersectTriangle (cuda/include/RayIntersection.cuh:54-111) on float32
    arrays that broadcast against each other (last axis xyz).  Returns (ok,
    dist, u, v): ok where the reference returns (dist, u, v, 0), else it
    returns zeros."""
    c = lambda a: tuple(np.asarray(a[..., k], np.float32) for k in range(3))      # noqa: E731
    v0, v1, v2, o, d = c(v0), c(v1), c(v2), c(o), c(d)
    with np.errstate(all="ignore"):
        e1 = tuple(v1[k] - v0[k] for k in range(3))
        e2 = tuple(v2[k] - v0[k] for k in range(3))
        p = _cross(d, e2)
        det = _dot(e1, p)
        inv_det = F(1.0) / det
        t = tuple(o[k] - v0[k] for k in range(3))
        u = _dot(t, p) * inv_det
        q = _cross(t, e1)
        v = _dot(d, q) * inv_det
        dist = _dot(e2, q) * inv_det
        ok = ~((det > -EPS) & (det < EPS)) & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & (dist > EPS)
    for a in (det, u, v, dist):
        assert a.dtype == np.float32
    return ok, dist, u, v


def brute_force(V, origins, dirs, tmax=None):
    """Every ray against every triangle.  Returns (acc, dist, u, v), each
    (N, T): acc where the closest-hit update could accept the triangle
    (dist > eps and dist < tmax)."""
    o, d = origins[:, None, :], dirs[:, None, :]
    ok, dist, u, v = tri_test(V[None, :, 0], V[None, :, 1], V[None, :, 2], o, d)
    t0 = np.full(len(origins), NO_HIT, np.float32) if tmax is None else np.asarray(tmax, np.float32)
    with np.errstate(invalid="ignore"):
        acc = ok & (dist < t0[:, None])
    return acc, dist, u, v


def closest(acc, dist):
    """(hit, tmin) per ray from brute_force's output."""
    d = np.where(acc, dist, np.float32(np.inf)).astype(np.float32)
    tmin = d.min(1) if d.shape[1] else np.full(len(d), np.inf, np.float32)
    return acc.any(1), tmin


# ---- the ray set ---------------------------------------------------------------------
def ray_set(V, n, seed=SEED):
    """n rays against the triangles V (T,3,3), a share of each kind, in a
    fixed order: 'aim' (origins outside the bounds aimed at centroids: certain
    hits on a triangle with area), 'random', 'axis' (axis-aligned directions
    with exact zeros, through a centroid), 'half' and 'triple' (aimed
    directions scaled by 0.5 and 3), 'on' (origins on a triangle), 'below'
    (aimed, tmax half the nearest hit: must miss) and 'between' (aimed, tmax
    between the first and the second hit, or twice the first: must return the
    first).  Returns dict origins, dirs (n,3), tmax (n,), kind (n,) str."""
    rng = np.random.default_rng(seed)
    T = len(V)
    lo, hi = V.reshape(-1, 3).min(0), V.reshape(-1, 3).max(0)
    ext = np.maximum(hi - lo, 1.0)
    cen = (V[:, 0].astype(np.float64) + V[:, 1] + V[:, 2]) / 3.0
    kinds = ["aim", "random", "axis", "half", "triple", "on", "below", "between"]
    kind = np.array([kinds[i % len(kinds)] for i in range(n)])
    o = np.zeros((n, 3))
    d = np.zeros((n, 3))
    for i in range(n):
        k = kind[i]
        tri = int(rng.integers(0, T))
        side = rng.normal(0, 1, 3)
        side /= np.linalg.norm(side)
        outside = (lo + hi) / 2 + side * np.linalg.norm(ext) * rng.uniform(0.8, 1.6)
        if k == "random":
            o[i] = rng.uniform(lo - ext, hi + ext)
            d[i] = rng.normal(0, 1, 3)
        elif k == "axis":
            ax, sign = int(rng.integers(0, 3)), rng.choice([-1.0, 1.0])
            o[i] = np.float32(cen[tri])
            o[i, ax] -= sign * ext[ax] * 1.5
            d[i, ax] = sign
        elif k == "on":
            w = rng.dirichlet([1, 1, 1])
            o[i] = w @ V[tri].astype(np.float64)
            d[i] = rng.normal(0, 1, 3)
        else:
            o[i] = outside
            d[i] = cen[tri] - np.float32(outside).astype(np.float64)
            if k == "half":
                d[i] *= 0.5
            if k == "triple":
                d[i] *= 3.0
    o, d = o.astype(np.float32), d.astype(np.float32)
    tmax = np.full(n, NO_HIT, np.float32)
    acc, dist, _, _ = brute_force(V, o, d)
    for i in np.flatnonzero((kind == "below") | (kind == "between")):
        ts = np.unique(dist[i][acc[i]])
        if len(ts) == 0:
            continue
        if kind[i] == "below":
            tmax[i] = ts[0] * F(0.5)
        else:
            tmax[i] = (ts[0] + ts[1]) * F(0.5) if len(ts) > 1 and (ts[0] + ts[1]) * F(0.5) > ts[0] else ts[0] * F(2.0)
    return dict(origins=o, dirs=d, tmax=tmax, kind=kind)


# ---- an independent ordering: depth first, near child first ----------------------------
def _bits(x):
    return int(np.float32(x).view(np.int32))


def _float(i):
    return np.int32(i).view(np.float32)


def _fmin(a, b):
    """fminf as the reference's GPU evaluates it: a NaN operand is ignored, -0 < +0."""
    if a != a:
        return b
    if b != b:
        return a
    if a < b or b < a:
        return a if a < b else b
    return a if np.signbit(a) else b


def _fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    if a > b or b > a:
        return a if a > b else b
    return b if np.signbit(a) else a


# The NaN of an invalid operation (inf - inf): the device makes it with the
# sign bit set (test_gpu_extreme.py pins that), as x86 and numpy on it do;
# other hosts clear it, and the integer comparisons below read that bit.  The
# span is the device's on any host.
DEVICE_NAN = np.uint32(0xFFC00000).view(np.float32)


def _span(n, ch, o, inv):
    """(entry, exit) of the ray's line in child ch's box of node rows n (4,4),
    clamped to [0, 1e20]: spanBeginKepler / spanEndKepler
    (MathHelpers.cuh:454-552) on the reference's float32 slab arithmetic: a
    float min / max per axis for x and y, then an integer max / min over the
    bit patterns, into which z and the clamp enter as integers only."""
    if ch == 0:
        b = [(n[0, 0], n[0, 1]), (n[0, 2], n[0, 3]), (n[2, 0], n[2, 1])]
    else:
        b = [(n[1, 0], n[1, 1]), (n[1, 2], n[1, 3]), (n[2, 2], n[2, 3])]
    t = []
    for a in range(3):
        od = F(o[a] * inv[a])
        pair = [F(F(b[a][0] * inv[a]) - od), F(F(b[a][1] * inv[a]) - od)]
        t.append([DEVICE_NAN if x != x else x for x in pair])
    (x0, x1), (y0, y1), (z0, z1) = t
    zb = max(min(_bits(z0), _bits(z1)), _bits(F(0.0)))
    ze = min(max(_bits(z0), _bits(z1)), _bits(NO_HIT))
    lo = _float(max(_bits(_fmin(x0, x1)), _bits(_fmin(y0, y1)), zb))
    hi = _float(min(_bits(_fmax(x0, x1)), _bits(_fmax(y0, y1)), ze))
    return lo, hi


def dfs_slots(flat, o, d):
    """The triangle slots in the order a depth-first walk of the flat tree
    tests them for this ray: only boxes the ray's line pierces, the nearer
    child first, child 0 on equal entries, leaf slots in order.  The spans
    are the reference's (_span), NaN and signed zeros included."""
    bvh = np.asarray(flat["bvh"], np.float32).reshape(-1, 4, 4)
    vx = u32(flat["verts"][:, 0])
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        inv = np.array([F(1.0) / (d[a] if abs(d[a]) > EPS else EPS) for a in range(3)], np.float32)
    out = []

    def child(idx):
        if idx >= 0:
            node(idx // 4)
            return
        s = ~idx
        while vx[s] != TERM:
            out.append(s)
            s += 3

    def node(i):
        n = bvh[i]
        idx = n[3, :2].copy().view(np.int32)
        with np.errstate(all="ignore"):
            (a0, b0), (a1, b1) = _span(n, 0, o, inv), _span(n, 1, o, inv)
        order = [c for c in ((1, 0) if a1 < a0 else (0, 1)) if (b0 >= a0 if c == 0 else b1 >= a1)]
        for c in order:
            child(int(idx[c]))

    node(0)
    return out


# ---- a hand-made deep tree ---------------------------------------------------------------
def chain_tree(levels=40):
    """A flat tree that is one chain of `levels` inner nodes: node i holds
    triangle i in a leaf (child 0) and node i + 1 (child 1), the last node two
    leaves: levels + 1 triangles along x, exact boxes."""
    rng = np.random.default_rng(11)
    T = levels + 1
    V = (rng.uniform(-1, 1, (T, 3, 3)) + np.array([3.0, 0, 0]) * np.arange(T)[:, None, None]).astype(np.float32)
    verts = np.zeros((4 * T, 4), np.float32)
    for t in range(T):
        verts[4 * t:4 * t + 3, :3] = V[t]
        verts[4 * t + 3, 0] = np.array([TERM], np.uint32).view(np.float32)[0]
    bvh = np.zeros((levels, 4, 4), np.float32)
    words = bvh.view(np.int32)
    for i in range(levels):
        rest = V[i + 1:].reshape(-1, 3)
        own = V[i]
        bvh[i, 0] = [own[:, 0].min(), own[:, 0].max(), own[:, 1].min(), own[:, 1].max()]
        bvh[i, 1] = [rest[:, 0].min(), rest[:, 0].max(), rest[:, 1].min(), rest[:, 1].max()]
        bvh[i, 2] = [own[:, 2].min(), own[:, 2].max(), rest[:, 2].min(), rest[:, 2].max()]
        words[i, 3, 0] = ~(4 * i)
        words[i, 3, 1] = 4 * (i + 1) if i + 1 < levels else ~(4 * (i + 1))
    z = np.zeros_like(verts)
    return dict(bvh=bvh.reshape(-1, 4), verts=verts, normals=z.copy(), tangents=z.copy(),
                uvs=np.zeros((4 * T, 2), np.float32))
