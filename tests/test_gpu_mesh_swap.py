"""One context taken through every way of replacing its mesh, in turn: a host
upload, a Morton device build, a host upload, a SAH device build, a refit, a
host upload.  After every step the context must be indistinguishable from a
fresh one loaded that single way -- what a swap of the resident mesh can get
wrong is an array or a scalar of the previous mesh going stale (the refit
arrays after a host upload, the depth that sizes the traversal stack, the
counts behind the export and vrhip_bvh_info, what a ray query reports as prim)."""
import numpy as np
import pytest

from device_mesh_cases import bitexact, deform, device_build
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, flat_trace_rays, scenes

pytestmark = pytest.mark.gpu

TIMES = [4242, 4249]
WALK = ["host", "morton", "host", "sah", "refit", "host"]
MAX_LEAF = {"morton": 3, "sah": 2}                  # the host tree has leaves of 2: three shapes in the walk


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda(0)


def rays_at(mesh, moved, n=12):
    """n fixed rays from a ring around the knot, each through the centroid of
    a triangle: the even ones of the knot as built, the odd ones of the moved
    knot, so at least half of them hit whichever of the two is resident."""
    tris = mesh["tris"].astype(np.int64)[np.linspace(0, len(mesh["tris"]) - 1, n).astype(np.int64)]
    cen = np.where(np.arange(n)[:, None] % 2 == 0, np.asarray(mesh["positions"], np.float64)[tris].mean(1),
                   np.asarray(moved, np.float64)[tris].mean(1))
    a = 2.0 * np.pi * np.arange(n) / n
    o = np.stack([140.0 * np.cos(a), 30.0 * np.sin(3 * a), 140.0 * np.sin(a)], -1)
    return o.astype(np.float32), (cen - o).astype(np.float32)


def apply(r, step, mesh, moved):
    if step == "host":
        r.initMesh(scenes.knot_flat(40, 20))
    elif step == "refit":                           # of the SAH tree the step before built
        r.refitMeshDevice(dev(moved))
    else:
        device_build(r, mesh, MAX_LEAF[step], step)


def observe(r, rays):
    """Everything the mesh shows through the API, the 2-frame accumulation last."""
    out = dict(flat=r.export_mesh_flat(), info=r.bvh_info())
    hits = r.traceRays(dev(rays[0]), dev(rays[1]))
    out["hits"] = {k: v.cpu().numpy() for k, v in hits.items()}
    r.clearBuffer()
    r.render(frames=len(TIMES), times=TIMES)
    out["accum"] = r.read_accum()
    return out


def fresh_context(sc):
    r = VRendererHIP(0)
    scenes.load_into(r, dict(sc, mesh_flat=None))
    return r


def test_every_swap_leaves_what_a_fresh_context_holds(native):
    mesh = scenes.torus_knot(40, 20)
    assert len(mesh["tris"]) == 1600
    P = mesh["positions"]
    moved = deform(P)
    rays = rays_at(mesh, moved)
    sc = scenes.make_scene("C2", 64, 48, knot=(40, 20))

    want = {}                                       # per way of loading, from a context that did nothing else
    for step in ("host", "morton", "sah", "refit"):
        f = fresh_context(sc)
        if step == "refit":
            apply(f, "sah", mesh, moved)
        apply(f, step, mesh, moved)
        want[step] = observe(f, rays)
        f.cleanUp()
    # not vacuous: three tree shapes, and the refit shows in the image
    assert len({w["info"] for w in want.values()}) >= 2 and want["morton"]["info"] != want["host"]["info"]
    assert np.any(want["refit"]["accum"] != want["sah"]["accum"])

    r = fresh_context(sc)
    for i, step in enumerate(WALK):
        what = f"step {i} ({step})"
        apply(r, step, mesh, moved)
        if step == "host":                          # no index data: refused, and nothing written
            with pytest.raises(VRHIPError) as e:
                r.refitMeshDevice(dev(moved))
            assert e.value.code == -1, what
        got, w = observe(r, rays), want[step]
        for k in w["flat"]:
            assert got["flat"][k].tobytes() == w["flat"][k].tobytes(), f"{what}: {k}"
        assert got["info"] == w["info"], what
        for k in ("t", "prim", "u", "v"):
            assert got["hits"][k].tobytes() == w["hits"][k].tobytes(), f"{what}: {k}"
        bitexact(got["accum"], w["accum"], what)
        # what prim names: the host walk over the export gives the flat slot of every hit
        walk = flat_trace_rays(got["flat"], rays[0], rays[1])
        hit = walk["prim"] >= 0
        assert hit.sum() >= 6 and ((got["hits"]["prim"] >= 0) == hit).all(), what
        if step == "host":
            assert (got["hits"]["prim"] == walk["prim"]).all(), what
        else:                                       # the caller's triangle, at the positions the mesh now has
            V = (moved if step == "refit" else P)[mesh["tris"].astype(np.int64)][got["hits"]["prim"][hit]]
            held = np.stack([got["flat"]["verts"][walk["prim"][hit] + k, :3] for k in range(3)], 1)
            assert held.tobytes() == V.tobytes(), what
        if step == "morton":                        # a device-built mesh takes a refit
            r.refitMeshDevice(dev(moved))
    r.cleanUp()
