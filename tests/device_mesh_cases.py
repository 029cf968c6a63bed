"""Meshes, builds and comparisons shared by the device-mesh GPU tests
(test_gpu_device_build.py, test_gpu_device_sah.py, test_gpu_refit.py,
test_gpu_devmesh_digests.py), and the cases and digests of the recorded
fixture tests/golden/devmesh_digests.json (tests/golden/gen_devmesh_digests.py)."""
import hashlib

import numpy as np

from vrenderer_pathtracer_amd import VRendererHIP, scenes

BUILDERS = ["morton", "sah"]
HARD_KINDS = ["identical", "equal_centres", "zero_area", "flat_axis", "far", "shared", "no_attributes"]


# ---- meshes -----------------------------------------------------------------
def soup(n, seed=5, spread=30.0, sigma=4.0):
    """The generator of test_capi.test_random_soup_bvh_equals_brute_force."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3))
    P = (c + rng.normal(0, sigma, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return dict(positions=P, normals=rng.normal(0, 1, (3 * n, 3)).astype(np.float32),
                tangents=rng.normal(0, 1, (3 * n, 3)).astype(np.float32),
                uvs=rng.uniform(0, 1, (3 * n, 2)).astype(np.float32),
                tris=np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))


def hard_mesh(kind):
    if kind == "identical":
        m = soup(1, seed=2, spread=5.0, sigma=12.0)
        return {k: np.tile(v, (50, 1)) if k != "tris" else np.arange(150, dtype=np.uint32).reshape(-1, 3)
                for k, v in m.items()}
    if kind == "equal_centres":
        base = np.array([[-1, -1, -1], [1, -1, 1], [0, 1, 0]], np.float32)     # box [-1, 1]^3
        m = soup(40, seed=3)
        m["positions"] = np.concatenate([base * np.float32(2.0 + 0.25 * i) for i in range(40)]).astype(np.float32)
        return m
    if kind == "zero_area":
        m = soup(60, seed=4)
        P = m["positions"].reshape(-1, 3, 3)
        P[::3, 1] = P[::3, 0]                                                  # two equal vertices
        P[1::6, 1] = P[1::6, 0]
        P[1::6, 2] = P[1::6, 0]                                                # a point
        return m
    if kind == "flat_axis":
        m = soup(80, seed=6)
        m["positions"][:, 2] = 0.0
        return m
    if kind == "far":
        return soup(80, seed=7, spread=1e5, sigma=3e4)
    if kind == "shared":
        return scenes.torus_knot(40, 20)
    if kind == "no_attributes":
        m = scenes.torus_knot(40, 20)
        return dict(positions=m["positions"], tris=m["tris"])
    raise ValueError(kind)


def deform(P, k=0.03, shift=(12, -8, 5)):
    """Twist about y by k*y rad, then shift: float64 math, the result as
    float32 (the test holds the exact fp32 positions the device gets).  The
    knot spans about +-50 and the camera sits at z = 150, so it stays in view."""
    P = np.asarray(P, np.float64)
    a = k * P[:, 1]
    c, s = np.cos(a), np.sin(a)
    out = np.stack([c * P[:, 0] + s * P[:, 2], P[:, 1], -s * P[:, 0] + c * P[:, 2]], -1)
    return (out + np.asarray(shift, np.float64)).astype(np.float32)


# ---- builds -------------------------------------------------------------------
def device_build(r, mesh, max_leaf=2, builder=None, **kw):
    """builder None: initMeshDevice without the argument (its default)."""
    import torch
    dev = torch.device("cuda", 0)

    def t(a, dtype):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to(dev)
    if builder is not None:
        kw["builder"] = builder
    r.initMeshDevice(t(mesh["positions"], np.float32), t(mesh["tris"], np.int32), t(mesh.get("normals"), np.float32),
                     t(mesh.get("tangents"), np.float32), t(mesh.get("uvs"), np.float32), max_leaf_tris=max_leaf, **kw)


def fresh(w=64, h=48):
    r = VRendererHIP(0)
    r.init(w, h)
    return r


def built_export(mesh, max_leaf=2, builder=None):
    r = fresh()
    device_build(r, mesh, max_leaf, builder)
    flat, info = r.export_mesh_flat(), r.bvh_info()
    r.cleanUp()
    return flat, info


def loaded(sc, mesh, builder=None):
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    device_build(r, mesh, 2, builder)
    return r


# ---- comparisons ----------------------------------------------------------------
def expected_triangles(mesh):
    """Per input triangle, its 3 x (position, normal, tangent, uv) as one row."""
    tris = np.asarray(mesh["tris"], np.int64)
    nv = len(mesh["positions"])
    cols = [np.asarray(mesh["positions"], np.float32)[tris]]
    for key, k in (("normals", 3), ("tangents", 3), ("uvs", 2)):
        a = mesh.get(key)
        a = np.zeros((nv, k), np.float32) if a is None else np.asarray(a, np.float32)
        cols.append(a[tris])
    rows = np.ascontiguousarray(np.concatenate(cols, -1).reshape(len(tris), -1))
    return np.concatenate([rows, rows]) if len(tris) == 1 else rows       # one triangle is stored twice


def sorted_rows(a):
    a = np.ascontiguousarray(a, np.float32) + np.float32(0.0)             # -0 -> +0: compare as floats
    return a[np.lexsort(a.T[::-1])]


def bitexact(g, o, what):
    diff = (g.view(np.uint32) != o.view(np.uint32)) if g.dtype == np.float32 else (g != o)
    n = int(diff.any(-1).sum())
    assert n == 0, f"{what}: {n} pixels differ (first at {np.argwhere(diff.any(-1))[:3].tolist()})"


# ---- the recorded digests -----------------------------------------------------------
def digest_cases():
    """{id: (mesh factory, max_leaf)}: 1 triangle is stored twice, 2 are a root
    with two leaves, 65 cross the SAH builder's one-wave limit (kSahSmall = 64),
    257 a 256-thread block."""
    cases = {f"soup{n}-leaf{leaf}": ((lambda n=n: soup(n)), leaf) for n in (1, 2, 5, 65, 257, 1000) for leaf in (1, 3)}
    cases.update({kind: ((lambda kind=kind: hard_mesh(kind)), 2) for kind in HARD_KINDS})
    cases["soup5-bare-leaf2"] = (lambda: {k: v for k, v in soup(5).items() if k in ("positions", "tris")}, 2)
    return cases


def digest_renderers():
    """One renderer per scene setting (C2, C3) at 64x48; every case replaces its mesh."""
    out = {}
    for name in ("C2", "C3"):
        out[name] = VRendererHIP(0)
        scenes.load_into(out[name], scenes.make_scene(name, 64, 48))
    return out


def _tree_digest(r):
    h = hashlib.sha256()
    flat = r.export_mesh_flat()
    for k in sorted(flat):
        h.update(f"{k} {flat[k].dtype} {flat[k].shape}\0".encode() + flat[k].tobytes())
    h.update(repr(tuple(int(v) for v in r.bvh_info())).encode())
    return h.hexdigest()


def _render_digest(renderers, times=(4242, 4249)):
    """2 frames per scene in both traversal modes: what reads bvh16 and tpath."""
    h = hashlib.sha256()
    for name in sorted(renderers):
        r = renderers[name]
        for strict in (False, True):
            r.set_strict_traversal(strict)
            r.clearBuffer()
            r.render(frames=len(times), times=list(times))
            h.update(r.read_accum().tobytes() + r.read_rgba8().tobytes() + r.read_depth8().tobytes())
        r.set_strict_traversal(False)
    return h.hexdigest()


def case_digests(renderers, builder, mesh, max_leaf):
    """SHA-256 of the exported tree and of the renders on it, as built and
    after a refit to deform(positions)."""
    import torch
    out = {}
    for r in renderers.values():
        device_build(r, mesh, max_leaf, builder)
    trees = {_tree_digest(r) for r in renderers.values()}
    assert len(trees) == 1                                 # the build does not depend on the scene
    out["tree"] = trees.pop()
    out["render"] = _render_digest(renderers)
    moved = torch.from_numpy(deform(mesh["positions"])).cuda(0)
    for r in renderers.values():
        r.refitMeshDevice(moved)
    trees = {_tree_digest(r) for r in renderers.values()}
    assert len(trees) == 1
    out["tree_refit"] = trees.pop()
    out["render_refit"] = _render_digest(renderers)
    return out
