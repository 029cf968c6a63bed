"""Ray queries against the resident mesh (vrhip_trace_rays, vr_rayquery.hip).
The oracle for the device is the host walk on what the device holds,
flat_trace_rays(r.export_mesh_flat(), ...) (checked against brute force in
test_ray_query_cpu.py): t, u, v and hit-or-miss bit for bit; the triangle's
identity through the data for a device-built mesh (prim is the caller's
triangle) and directly for a host upload (prim is the flat slot); strict and
culled walks equal each other bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

from device_mesh_cases import BUILDERS, deform, device_build, fresh, hard_mesh, soup
from ray_query_cases import NO_HIT, chain_tree, flat_triangles, ray_set, same_bits, u32
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, build_flat, flat_trace_rays, scenes

pytestmark = pytest.mark.gpu

N_RAYS = 1000
UPLOADS = BUILDERS + ["host"]
MESHES = {f"soup{n}-leaf{leaf}": ((lambda n=n: soup(n)), leaf) for n in (1, 2, 65, 1000) for leaf in (1, 3)}
MESHES.update({kind: ((lambda kind=kind: hard_mesh(kind)), 2) for kind in ("identical", "shared", "zero_area", "flat_axis",
                                                                             "far", "equal_centres", "no_attributes")})
FIELDS = ("t", "u", "v")


def dev(a, dtype=np.float32):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda(0)


def triangles_of(mesh, positions=None):
    P = mesh["positions"] if positions is None else positions
    return np.ascontiguousarray(np.asarray(P, np.float32)[mesh["tris"].astype(np.int64)])


@functools.lru_cache(maxsize=None)
def case(name):
    """(mesh, leaf, rays): computed once, shared by every test of the mesh, never written."""
    make, leaf = MESHES[name]
    mesh = make()
    return mesh, leaf, ray_set(triangles_of(mesh), N_RAYS)


@pytest.fixture(scope="module")
def r(native):
    r = fresh()
    yield r
    r.cleanUp()


def upload(r, mesh, leaf, how):
    """The flat arrays of a host upload, None for a device build."""
    if how == "host":
        flat = build_flat(mesh, leaf)
        r.initMesh(flat)
        return flat
    device_build(r, mesh, leaf, how)
    return None


def trace(r, rays, n=None, any_hit=False, tmax=True):
    n = len(rays["origins"]) if n is None else n
    out = r.traceRays(dev(rays["origins"][:n]), dev(rays["dirs"][:n]), dev(rays["tmax"][:n]) if tmax else None,
                      any_hit=any_hit)
    assert all(out[k].is_cuda for k in out) and out["prim"].dtype.is_floating_point is False
    return {k: v.cpu().numpy() for k, v in out.items()}


def host(flat, rays, n=None, any_hit=False, tmax=True):
    n = len(rays["origins"]) if n is None else n
    return flat_trace_rays(flat, rays["origins"][:n], rays["dirs"][:n], rays["tmax"][:n] if tmax else None, any_hit=any_hit)


def same_records(a, b, what):
    for k in FIELDS:
        bad = np.flatnonzero(u32(a[k]) != u32(b[k]))
        assert len(bad) == 0, f"{what}: {k} differs on {len(bad)} rays (first {bad[:5].tolist()})"
    assert ((a["prim"] >= 0) == (b["prim"] >= 0)).all(), what


def check_device_against_host(r, got, rays, mesh, uploaded_flat, what, positions=None, n=None):
    """got: the device's records; the host walk runs on the export."""
    flat = r.export_mesh_flat()
    want = host(flat, rays, n)
    same_records(got, want, what)
    hit = want["prim"] >= 0
    if uploaded_flat is not None:                       # a host upload: prim is the slot in the uploaded arrays
        assert all(uploaded_flat[k].tobytes() == flat[k].tobytes() for k in ("bvh", "verts"))
        assert (got["prim"] == want["prim"]).all(), what
    else:                                               # a device build: prim is the caller's triangle
        assert ((got["prim"][hit] >= 0) & (got["prim"][hit] < len(mesh["tris"]))).all()
        V = triangles_of(mesh, positions)[got["prim"][hit]]
        slot = want["prim"][hit]
        held = np.stack([flat["verts"][slot + k, :3] for k in range(3)], 1)
        assert held.tobytes() == V.tobytes(), what
    return want


# ---- 1. + 3. meshes x uploads, both walks --------------------------------------------------
@pytest.mark.parametrize("how", UPLOADS)
@pytest.mark.parametrize("name", list(MESHES))
def test_device_equals_host_walk(r, name, how):
    mesh, leaf, rays = case(name)
    flat = upload(r, mesh, leaf, how)
    got = {}
    for strict in (False, True):
        r.set_strict_traversal(strict)
        got[strict] = trace(r, rays)
    r.set_strict_traversal(False)
    same_records(got[False], got[True], f"{name} {how}: culled against strict")
    assert (got[False]["prim"] == got[True]["prim"]).all()
    want = check_device_against_host(r, got[True], rays, mesh, flat, f"{name} {how} strict")
    check_device_against_host(r, got[False], rays, mesh, flat, f"{name} {how} culled")
    if name.startswith("soup"):
        hit = want["prim"] >= 0
        assert hit[np.isin(rays["kind"], ["aim", "half", "triple", "between"])].all()
        assert not hit[rays["kind"] == "below"].any()
    # without tmax the closest so far starts at 1e20
    open_got, open_want = trace(r, rays, 128, tmax=False), host(r.export_mesh_flat(), rays, 128, tmax=False)
    same_records(open_got, open_want, f"{name} {how} without tmax")
    assert same_bits(open_got["t"][open_got["prim"] < 0], np.full((open_got["prim"] < 0).sum(), NO_HIT, np.float32))


# ---- 2. ray counts: the partial wave, the partial block, the grid-stride tail ------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_ray_counts(r, n):
    mesh, leaf, rays = case("soup65-leaf3")
    upload(r, mesh, leaf, "sah")
    check_device_against_host(r, trace(r, rays, n), rays, mesh, None, f"{n} rays", n=n)


# ---- 4. after a refit -----------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
def test_after_a_refit(r, builder):
    mesh, leaf, _ = case("shared")
    moved = deform(mesh["positions"])
    rays = ray_set(triangles_of(mesh, moved), 512)
    device_build(r, mesh, leaf, builder)
    r.refitMeshDevice(dev(moved))
    for strict in (False, True):
        r.set_strict_traversal(strict)
        want = check_device_against_host(r, trace(r, rays), rays, mesh, None, f"refit {builder} strict={strict}", moved)
    r.set_strict_traversal(False)
    assert (want["prim"] >= 0).sum() > 256


# ---- 5. a deep tree: the 64-entry stack ------------------------------------------------------
def test_deep_chain_tree(r):
    flat = chain_tree(40)
    _, V = flat_triangles(flat)
    rays = ray_set(V, 512)
    r.initMesh(flat)
    assert r.bvh_info()[0] == 40
    for strict in (False, True):
        r.set_strict_traversal(strict)
        want = check_device_against_host(r, trace(r, rays), rays, None, flat, f"chain strict={strict}")
    r.set_strict_traversal(False)
    assert (want["prim"] >= 0).sum() > 128


# ---- 6. any-hit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("how", UPLOADS)
@pytest.mark.parametrize("name", ["soup1-leaf1", "soup1000-leaf3", "identical", "shared"])
def test_any_hit(r, name, how):
    mesh, leaf, rays = case(name)
    upload(r, mesh, leaf, how)
    for strict in (False, True):
        r.set_strict_traversal(strict)
        hit = trace(r, rays)["prim"] >= 0
        got = trace(r, rays, any_hit=True)
        assert ((got["prim"] >= 0) == hit).all()
        assert not got["prim"][hit].any() and not any(u32(got[k][hit]).any() for k in FIELDS)   # exactly {0,0,0,0}
        assert same_bits(got["t"][~hit], rays["tmax"][~hit]) and (got["prim"][~hit] == -1).all()
        assert not u32(got["u"][~hit]).any() and not u32(got["v"][~hit]).any()
    r.set_strict_traversal(False)
    assert 0 < hit.sum() < len(hit)


# ---- 7. output bounds ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_only_the_rays_rows_are_written(r, n):
    import torch
    mesh, leaf, rays = case("soup65-leaf3")
    upload(r, mesh, leaf, "morton")
    guard = 64
    rec = torch.full((n + 2 * guard, 4), 0x5A5AA5A5, dtype=torch.int32, device="cuda:0")
    o, d, t = dev(rays["origins"][:n]), dev(rays["dirs"][:n]), dev(rays["tmax"][:n])
    torch.cuda.synchronize()
    p = lambda x: ctypes.c_void_p(x.data_ptr() if n else 0)               # noqa: E731
    rc = r._lib.vrhip_trace_rays(r._ctx, p(o), p(d), p(t), n, 0, ctypes.c_void_p(rec.data_ptr() + 16 * guard))
    assert rc == 0
    out = rec.cpu().numpy()
    assert (out[:guard] == 0x5A5AA5A5).all() and (out[guard + n:] == 0x5A5AA5A5).all()
    if n:
        want = trace(r, rays, n)
        assert (out[guard:guard + n, 0].view(np.float32).view(np.uint32) == u32(want["t"])).all()
        assert (out[guard:guard + n] != 0x5A5AA5A5).any(1).all()


# ---- 8. non-finite rays ----------------------------------------------------------------------------
def test_non_finite_rays_in_a_batch(r):
    mesh, leaf, rays = case("soup1000-leaf3")
    upload(r, mesh, leaf, "sah")
    n = 256
    clean = trace(r, rays, n)
    bad = {k: v[:n].copy() for k, v in rays.items()}
    rows = np.arange(0, n, 7)
    for j, i in enumerate(rows):
        which = j % 5
        if which == 0:
            bad["origins"][i, j % 3] = np.nan
        elif which == 1:
            bad["dirs"][i, j % 3] = np.inf
        elif which == 2:
            bad["origins"][i, j % 3] = -np.inf
        elif which == 3:
            bad["dirs"][i] = np.nan
        else:
            bad["tmax"][i] = np.nan
    for strict in (False, True):
        r.set_strict_traversal(strict)
        for any_hit in (False, True):
            got = trace(r, bad, any_hit=any_hit)
            assert (got["prim"][rows] == -1).all() and same_bits(got["t"][rows], np.full(len(rows), NO_HIT, np.float32))
            assert not u32(got["u"][rows]).any() and not u32(got["v"][rows]).any()
            if not any_hit:
                rest = np.setdiff1d(np.arange(n), rows)
                assert all(same_bits(got[k][rest], clean[k][rest]) for k in FIELDS)
                assert (got["prim"][rest] == clean["prim"][rest]).all()
    r.set_strict_traversal(False)
    same_records(trace(r, bad), host(r.export_mesh_flat(), bad), "non-finite batch against the host")


# ---- 9. no side effects on rendering -------------------------------------------------------------------
@pytest.mark.parametrize("service", [False, True])
def test_a_query_leaves_the_render_alone(native, service):
    sc = scenes.make_scene("C2", 64, 48)
    mesh, leaf, rays = case("shared")
    images = {}
    for query in (False, True):
        q = VRendererHIP(0)
        scenes.load_into(q, sc)
        device_build(q, mesh, 2, "sah")
        if service:
            q.set_service(1)
        q.render(frames=2, times=[11, 12], sync=not service)
        if query:
            s0 = q.service_info()["sessions"]
            before = q.getFrameCount()
            got = trace(q, rays, 256)
            assert q.getFrameCount() == before == 2
            assert (got["prim"] >= 0).any()
        q.render(frames=2, times=[13, 14], sync=not service)
        q.sync()
        if query and service:
            assert q.service_info()["sessions"] > s0 >= 1                # the query closed the first session
        assert q.getFrameCount() == 4
        images[query] = (q.read_accum(), q.read_rgba8(), q.read_depth8())
        q.cleanUp()
    for a, b in zip(images[False], images[True]):
        assert a.tobytes() == b.tobytes()
    assert np.any(images[True][0][..., :3] != 0)


# ---- 10. refusals -------------------------------------------------------------------------------------------
def test_refusals(native):
    mesh, leaf, rays = case("soup65-leaf3")
    o, d, t = dev(rays["origins"][:64]), dev(rays["dirs"][:64]), dev(rays["tmax"][:64])
    q = fresh()                                          # no mesh
    with pytest.raises(VRHIPError) as e:
        q.traceRays(o, d)
    assert e.value.code == -1
    device_build(q, mesh, leaf, "morton")
    want = trace(q, rays, 64)
    assert q._lib.vrhip_trace_rays(q._ctx, ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(d.data_ptr()), None, 64, 2,
                                   ctypes.c_void_p(o.data_ptr())) == -1          # an unknown mode
    wrong = [dict(origins=o.cpu(), dirs=d), dict(origins=o, dirs=d.cpu()), dict(origins=o.double(), dirs=d),
             dict(origins=o, dirs=d.half()), dict(origins=o.t().contiguous().t(), dirs=d),
             dict(origins=o[:, :2].contiguous(), dirs=d), dict(origins=o, dirs=d[:-1]),
             dict(origins=o, dirs=d, tmax=t[:-1]), dict(origins=o, dirs=d, tmax=t.double()),
             dict(origins=o, dirs=d, tmax=t[:, None]), dict(origins=o, dirs=d, tmax=t.cpu()),
             dict(origins=o, dirs=d, tmax=dev(rays["tmax"][:128])[::2]), dict(origins=np.asarray(rays["origins"][:64]), dirs=d),
             dict(origins=None, dirs=d), dict(origins=o, dirs=None)]
    for kw in wrong:                                     # device, dtype, layout, shape, not a tensor, missing
        with pytest.raises(ValueError):
            q.traceRays(**kw)
    again = trace(q, rays, 64)
    assert all(same_bits(again[k], want[k]) for k in FIELDS) and (again["prim"] == want["prim"]).all()
    q.cleanUp()
    q = VRendererHIP([0])                                # a multi-device context of one device
    q.init(64, 48)
    with pytest.raises(VRHIPError) as e:
        q.traceRays(o, d)
    assert e.value.code == -1 and "multi-device" in str(e.value)
    q.cleanUp()
