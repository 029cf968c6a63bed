"""What the path tracer sees at the first hit of the caller's rays
(vrhip_trace_surface, vr_surface*.hip) and the camera's rays as a buffer
(vrhip_camera_rays).

The yardstick is the oracle's own intersect_scene (tests/surface_cases.py; tied
to the reference-pinned renders in test_surface_cpu.py): all 28 words of a
record equal it, compared as uint32, in both traversal modes, on camera rays
(set A), random rays (B), rays aimed at the mesh (C) and rays at the small
spheres and out of the scene (D).  Then the product against itself: a mesh
hit's (t, prim, barycentrics) is traceRays', the depth term of the position is
traceRadiance's w and the depth image, cameraRays() is the camera."""
import ctypes

import numpy as np
import pytest

import flag_lattice as fl
import radiance_cases as rc
import surface_cases as sf
from device_mesh_cases import deform, device_build, fresh
from vrenderer_pathtracer_amd import Camera, VRendererHIP, VRHIPError, scenes

pytestmark = pytest.mark.gpu

_live = {}


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda(0)      # a copy: the shared ray sets are read-only


def renderer(name, mesh="shallow"):
    """One renderer per scene for the whole module; the tests leave its scene
    flags as they found them."""
    key = (name, mesh)
    if key not in _live:
        r = VRendererHIP(0)
        scenes.load_into(r, sf.scene_named(name, mesh))
        _live[key] = r
    return _live[key]


@pytest.fixture(scope="module", autouse=True)
def _renderers(native):
    yield
    for r in _live.values():
        r.cleanUp()
    _live.clear()


def trace(r, o, d):
    """The [n, 28] records as uint32, and the dict's views checked against them."""
    import torch
    out = r.traceSurface(dev(o), dev(d))
    rec = out["record"]
    assert rec.is_cuda and tuple(rec.shape) == (len(o), 28) and rec.dtype == torch.float32
    for key, cols in (("position", sf.POSITION), ("normal", sf.NORMAL), ("tangent", sf.TANGENT), ("color", sf.COLOR),
                      ("specular", sf.SPECULAR), ("emission", sf.EMISSION)):
        assert tuple(out[key].shape) == (len(o), 3) and out[key].data_ptr() == rec[:, cols].data_ptr()
    for key, col in (("t", sf.T), ("kind", sf.KIND), ("prim", sf.PRIM), ("type", sf.TYPE)):
        assert tuple(out[key].shape) == (len(o),) and out[key].data_ptr() == rec[:, col].data_ptr()
        assert out[key].dtype == (torch.float32 if key == "t" else torch.int32)
    assert tuple(out["bary"].shape) == tuple(out["uv"].shape) == (len(o), 2)
    assert out["bary"].data_ptr() == rec[:, sf.BARY_U].data_ptr() and out["uv"].data_ptr() == rec[:, sf.TEX_U].data_ptr()
    assert out["bary"].stride() == out["uv"].stride() == (28, 4)
    return np.ascontiguousarray(rec.cpu().numpy()).view(np.uint32)


def same(got, want, what):
    bad = np.flatnonzero((got != want).any(-1))
    if len(bad):
        i = bad[0]
        words = np.flatnonzero(got[i] != want[i]).tolist()
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ (first {bad[:5].tolist()}; record {i} words "
                             f"{words}: {sf.floats(got[i:i + 1])[0, words].tolist()} against "
                             f"{sf.floats(want[i:i + 1])[0, words].tolist()}, kind {got[i, 1]} against {want[i, 1]})")


def same_or_nan(got, want, what):
    bad = np.flatnonzero(~sf.same_or_nan_in_both(got, want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ (first {bad[:5].tolist()})"


def check_against_yardstick(r, name, mesh, what):
    sc = sf.scene_named(name, mesh)
    for which in sf.sets_of(sc):
        o, d = sf.ray_set(which, sc)
        want, ok = sf.reference(name, which, mesh)
        got = trace(r, o, d)
        if sf.nan_case(name):
            assert ok.all()
            same_or_nan(got, want, f"{what} set {which}")
        else:
            same(got[ok], want[ok], f"{what} set {which}")


# ---- 1. parity with the yardstick ----------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("name", sf.COMBO_NAMES)
def test_parity_with_the_yardstick(oracle, name, strict):
    r = renderer(name)
    r.set_strict_traversal(strict)
    try:
        check_against_yardstick(r, name, "shallow", f"{name} strict={strict}")
    finally:
        r.set_strict_traversal(False)


# ---- 2. the deep mesh --------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
def test_parity_on_the_deep_mesh(oracle, strict):
    """24-entry stacks: the class kernel, and the generic one in strict mode."""
    name = "cornell+mesh"
    r = renderer(name, "deep")
    assert 15 < r.bvh_info()[0] <= 23
    r.set_strict_traversal(strict)
    try:
        check_against_yardstick(r, name, "deep", f"deep {name} strict={strict}")
    finally:
        r.set_strict_traversal(False)


# ---- 3. shading scenes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("name", sf.SHADING_NAMES)
def test_parity_on_shading_scenes(oracle, name, strict):
    """Maps of odd shapes, zero tangents, the example sphere with maps, and a
    scene with NaN normals (tests/shading_cases.py)."""
    r = renderer(name)
    r.set_strict_traversal(strict)
    try:
        check_against_yardstick(r, name, "shallow", f"{name} strict={strict}")
    finally:
        r.set_strict_traversal(False)


# ---- 4. device-built meshes ----------------------------------------------------------------------------
def slot_triangles(flat, slots):
    v = np.asarray(flat["verts"], np.float32).reshape(-1, 4)[:, :3]
    return np.stack([v[slots], v[slots + 1], v[slots + 2]], 1)


def check_device_mesh(q, sc, mesh, positions, what):
    """The record equals the yardstick on the exported tree, a word equal or
    NaN in both (no tangents: the tangent of a mesh hit is normalize(0)); prim
    is the row of tris, whose vertices are the hit slot's."""
    sc = dict(sc, mesh_flat=q.export_mesh_flat())
    tris = np.asarray(mesh["tris"], np.int64)
    records = []
    for which in ("B", "C"):
        o, d = sf.ray_set(which, sc) if which == "B" else sf.aimed_rays(sc["mesh_flat"], 256)
        want = sf.yardstick(sc, o, d)
        got = trace(q, o, d)
        m = want[:, sf.KIND] == sf.MESH
        assert (got[:, sf.KIND] == want[:, sf.KIND]).all(), what
        assert m.sum() >= (200 if which == "C" else 16), f"{what}: {m.sum()} mesh hits in set {which}"
        rows = got[m, sf.PRIM].astype(np.int64)
        assert (rows < len(tris)).all(), what
        mine = np.asarray(positions, np.float32)[tris[rows]]
        theirs = slot_triangles(sc["mesh_flat"], want[m, sf.PRIM].astype(np.int64))
        assert (np.sort(sf.u32(mine).reshape(len(rows), -1), -1) == np.sort(sf.u32(theirs).reshape(len(rows), -1), -1)).all(), what
        masked = got.copy()
        masked[m, sf.PRIM] = want[m, sf.PRIM]
        same_or_nan(masked, want, f"{what} set {which}")
        assert np.isnan(sf.floats(got)[m][:, sf.TANGENT]).all() and not got[m][:, [sf.TEX_U, sf.TEX_V]].any()
        f = sf.floats(got).copy()
        f[:, sf.TANGENT] = 0.0
        f[:, [sf.KIND, sf.PRIM, sf.TYPE]] = 0.0
        assert np.isfinite(f).all(), what
        records.append(got)
    return records


@pytest.mark.parametrize("builder,name", [("morton", "cornell+mesh"), ("sah", "mesh+tex_d+tex_n+tex_s")])
def test_device_meshes(oracle, builder, name):
    combo = rc.combo_of(name)
    sc = fl.scene_of(combo[:3] + (0,) + combo[4:])      # the mesh comes from the device build
    full = scenes.torus_knot(40, 20)
    mesh = dict(positions=full["positions"], tris=full["tris"])           # no normals, tangents or uvs
    q = VRendererHIP(0)
    scenes.load_into(q, sc)
    try:
        device_build(q, mesh, 2, builder)
        first = check_device_mesh(q, sc, mesh, mesh["positions"], f"{builder} built")
        moved = deform(mesh["positions"])
        q.refitMeshDevice(dev(moved))
        check_device_mesh(q, sc, mesh, moved, f"{builder} refit")
        q.refitMeshDevice(dev(mesh["positions"]))
        back = check_device_mesh(q, sc, mesh, mesh["positions"], f"{builder} refit back")
        for a, b in zip(first, back):
            same_or_nan(b, a, f"{builder}: refit back against the build")
    finally:
        q.cleanUp()


# ---- 5. consistency with traceRays -------------------------------------------------------------------------
@pytest.mark.parametrize("name,mesh", [("cornell+mesh", "shallow"), ("mesh+tex_d+tex_n+tex_s", "shallow"), ("cornell+mesh", "deep")])
def test_mesh_hits_are_trace_rays_hits(name, mesh):
    r = renderer(name, mesh)
    sc = sf.scene_named(name, mesh)
    n_mesh = 0
    for which in sf.sets_of(sc):
        o, d = sf.ray_set(which, sc)
        got = trace(r, o, d)
        m = got[:, sf.KIND] == sf.MESH
        n_mesh += int(m.sum())
        w = r.traceRays(dev(o), dev(sf.normalised(d)))
        t, prim, u, v = (w[k].cpu().numpy() for k in ("t", "prim", "u", "v"))
        assert (got[m, sf.T] == sf.u32(t[m])).all() and (got[m, sf.PRIM] == prim[m].astype(np.uint32)).all()
        assert (got[m, sf.BARY_U] == sf.u32(u[m])).all() and (got[m, sf.BARY_V] == sf.u32(v[m])).all()
        # a ray whose closest hit is a sphere: the mesh, if it is hit at all, lies behind it
        s = ~m & (got[:, sf.KIND] != sf.NONE)
        assert (t[s] >= sf.floats(got)[s, sf.T]).all()
        assert (prim[got[:, sf.KIND] == sf.NONE] == -1).all()
    assert n_mesh >= 400


# ---- 6. consistency with traceRadiance and the render ----------------------------------------------------
@pytest.mark.parametrize("name", sf.COMBO_NAMES)
def test_depth_term_is_the_radiance_query_s_and_the_render_s(name):
    import torch
    r = renderer(name)
    sc = sf.scene_named(name)
    o, d = r.cameraRays()
    out = r.traceSurface(o, d)
    rec = np.ascontiguousarray(out["record"].cpu().numpy()).view(np.uint32)
    hit = rec[:, sf.KIND] != sf.NONE
    l = o.cpu().numpy() - sf.floats(rec)[:, sf.POSITION]
    want = np.sqrt((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2]) / np.float32(150.0)
    assert want.dtype == np.float32
    want[~hit] = 0.0 if sc["cornell"] else 1.0
    t = 40503
    seeds = torch.from_numpy(rc.camera_seeds(sc, time=t).view(np.int32)).cuda(0)
    w = r.traceRadiance(o, d, seeds, samples=2).cpu().numpy()[:, 3]
    # a path that left the Cornell box after its first hit returns w = 0 (PathTracer.cu:649-652)
    escaped = hit & (w == 0.0) if sc["cornell"] else np.zeros(len(w), bool)
    assert escaped.sum() <= 4
    assert (sf.u32(w[~escaped]) == sf.u32(want[~escaped])).all(), name
    r.clearBuffer()
    r.render(frames=1, times=[t])
    depth = r.read_depth8()[..., 0].reshape(-1)
    r.clearBuffer()
    assert (depth[~escaped] == rc.depth_byte(want)[~escaped]).all() and (depth[escaped] == 255).all(), name
    assert hit.all() if sc["cornell"] else (hit.sum() >= 30 and (~hit).sum() >= 30)


# ---- 7. camera rays ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(32, 32), (37, 19)])
def test_camera_rays(w, h):
    q = VRendererHIP(0)
    q.init(w, h)
    try:
        poses = [scenes.default_camera(),
                 dict(origin=(12.5, -3.0, 90.0), dir=(-0.2, 0.1, -0.97), up=(0.05, 0.99, 0.1), right=(0.98, -0.04, -0.2),
                      fov_scale=0.61)]
        for cam in poses:
            q.setCamera(Camera(cam["origin"], cam["dir"], cam["up"], cam["right"], cam["fov_scale"]))
            o, d = q.cameraRays()
            assert o.is_cuda and tuple(o.shape) == tuple(d.shape) == (w * h, 3)
            want = rc.camera_dirs(dict(camera=cam, width=w, height=h))
            assert (sf.u32(d.cpu().numpy()) == sf.u32(want)).all(), (w, h)
            assert (sf.u32(o.cpu().numpy()) == sf.u32(np.tile(np.asarray(cam["origin"], np.float32), (w * h, 1)))).all()
        assert len(np.unique(sf.u32(want), axis=0)) == w * h
    finally:
        q.cleanUp()


# ---- 8. tails and invalid rays -------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("n", [1, 63, 65, 193])
def test_tails_and_invalid_rays(oracle, n, strict):
    import torch
    name = "cornell+mesh"
    r = renderer(name)
    o, d = (a[:n].copy() for a in sf.ray_set("B"))
    want, ok = sf.reference(name, "B")
    p = lambda x: ctypes.c_void_p(x.data_ptr())                            # noqa: E731

    def call(o, d):
        out = torch.full((n + 3, 28), -7.0, dtype=torch.float32, device="cuda:0")        # canary rows after row n
        do, dd = dev(o), dev(d)
        torch.cuda.synchronize()
        assert r._lib.vrhip_trace_surface(r._ctx, p(do), p(dd), n, p(out)) == 0
        got = np.ascontiguousarray(out.cpu().numpy()).view(np.uint32)
        assert (got[n:] == sf.u32(np.float32(-7.0))).all(), "rows past n_rays were written"
        return got[:n]

    r.set_strict_traversal(strict)
    try:
        clean = call(o, d)
        same(clean[ok[:n]], want[:n][ok[:n]], f"{n} rays")
        if n == 193:
            rows = np.arange(0, n, 5)
            for k, i in enumerate(rows):                # in rotation: a NaN, an inf, a zero direction, components of 3e38
                if k % 4 == 0:
                    o[i, k % 3] = np.nan
                elif k % 4 == 1:
                    d[i, k % 3] = -np.inf if k % 8 == 1 else np.inf
                elif k % 4 == 2:
                    d[i] = 0.0
                else:
                    d[i] = (3e38, -3e38, 3e38)
            got = call(o, d)
            assert not got[rows].any(), "an invalid ray's record is 28 zero words"
            rest = np.setdiff1d(np.arange(n), rows)
            same(got[rest], clean[rest], "the valid rays of the batch")
            assert clean[rows].any(-1).all()
    finally:
        r.set_strict_traversal(False)


def test_more_rays_than_a_resident_set(oracle):
    import torch
    name = "cornell+example"
    # the launcher's resident set: VR_SPHERE_MIN_WAVES (6) blocks of 256 rays on each CU
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (6 * cus + 3) * 256 + 77
    o, d = sf.ray_set("A")
    idx = np.arange(n) % len(o)
    got = trace(renderer(name), o[idx], d[idx])
    same(got, got[idx], "record i against record i mod 1024")
    want, ok = sf.reference(name, "A")
    same(got[:len(o)][ok], want[ok], "the first 1,024 records")


# ---- 9. state ----------------------------------------------------------------------------------------------------
def test_a_call_leaves_everything_else_alone():
    name = "cornell+mesh"
    sc = sf.scene_named(name)
    o, d = sf.ray_set("B")
    state = {}
    for query in (False, True):
        q = VRendererHIP(0)
        scenes.load_into(q, sc)
        q.render(frames=2, times=[11, 12])
        before = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount(), q.export_mesh_flat())
        if query:
            a, b = trace(q, o, d), trace(q, o, d)
            same(a, b, "two calls")
            q.cameraRays()
            after = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount(), q.export_mesh_flat())
            for x, y in zip(before[:3], after[:3]):
                assert x.tobytes() == y.tobytes()
            assert before[3] == after[3] == 2
            assert all(before[4][k].tobytes() == after[4][k].tobytes() for k in before[4])
        q.render(frames=1, times=[13])
        state[query] = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount())
        q.cleanUp()
    for x, y in zip(state[False][:3], state[True][:3]):
        assert x.tobytes() == y.tobytes()
    assert state[False][3] == state[True][3] == 3


@pytest.mark.parametrize("call", ["traceSurface", "cameraRays"])
def test_between_unsynchronised_renders_of_a_session(oracle, call):
    name = "cornell+mesh"
    sc = sf.scene_named(name)
    o, d = sf.ray_set("B")
    want, ok = sf.reference(name, "B")
    images = {}
    for query in (False, True):
        q = VRendererHIP(0)
        scenes.load_into(q, sc)
        q.set_service(1)
        q.render(frames=2, times=[11, 12], sync=False)
        if query:
            s0 = q.service_info()["sessions"]
            if call == "traceSurface":
                same(trace(q, o, d)[ok], want[ok], "inside a session")
            else:
                cd = q.cameraRays()[1].cpu().numpy()
                assert (sf.u32(cd) == sf.u32(rc.camera_dirs(sc))).all()
        q.render(frames=2, times=[13, 14], sync=False)
        q.sync()
        if query:
            assert q.service_info()["sessions"] > s0 >= 1        # the call closed the first session
        assert q.getFrameCount() == 4
        images[query] = (q.read_accum(), q.read_rgba8(), q.read_depth8())
        q.cleanUp()
    for a, b in zip(images[False], images[True]):
        assert a.tobytes() == b.tobytes()
    assert np.any(images[True][0][..., :3] != 0)


def test_scene_toggles(oracle):
    """useCornellBox / useExampleSphere on one renderer: the other
    combinations' yardsticks, the mesh ignored while the example sphere is on."""
    base = sf.scene_named("cornell+mesh")
    q = VRendererHIP(0)
    scenes.load_into(q, base)
    try:
        for cornell, example in ((True, True), (False, True), (False, False), (True, False)):
            q.useCornellBox(cornell)
            q.useExampleSphere(example)
            sc = dict(base, cornell=cornell, example_sphere=example)
            kinds = set()
            for which in ("B", "D"):
                o, d = sf.ray_set(which)
                want = sf.yardstick(sc, o, d)
                ok = sf.kept(want)
                same(trace(q, o, d)[ok], want[ok], f"cornell={cornell} example={example} set {which}")
                kinds |= set(np.unique(want[:, sf.KIND]).tolist())
            assert (sf.EXAMPLE in kinds) == example and (sf.MESH in kinds) == (not example) and (sf.CORNELL in kinds) == cornell
    finally:
        q.cleanUp()


# ---- 10. errors -----------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    o, d = (dev(a[:64]) for a in sf.ray_set("B"))
    p = lambda x: ctypes.c_void_p(x.data_ptr())                            # noqa: E731
    q = VRendererHIP([0])                                # a multi-device context of one device
    q.init(64, 48)
    for fn in (lambda: q.traceSurface(o, d), q.cameraRays):
        with pytest.raises(VRHIPError) as e:
            fn()
        assert e.value.code == -1 and "multi-device" in str(e.value)
    q.cleanUp()
    q = fresh()                                          # HDRI mode, no environment
    try:
        with pytest.raises(VRHIPError) as e:
            q.traceSurface(o, d)
        assert e.value.code == -3
        with pytest.raises(VRHIPError) as e:
            q.traceRadiance(o, d)
        assert e.value.code == -3                        # exactly where the radiance query refuses
        assert tuple(q.traceSurface(o[:0], d[:0])["record"].shape) == (0, 28)    # nothing to do comes first
        co, cd = q.cameraRays()                          # the camera needs no environment
        assert tuple(cd.shape) == (64 * 48, 3)
        q.useCornellBox(True)                            # a scene without a mesh
        want = q.traceSurface(o, d)["record"].cpu().numpy()
        assert sf.finite(sf.u32(want)).all() and np.any(want[:, sf.COLOR] != 0)
        out = torch.zeros((65, 28), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        L = q._lib
        assert L.vrhip_trace_surface(q._ctx, p(o), p(d), 64, ctypes.c_void_p(out.data_ptr() + 4)) == -1
        assert b"16-byte" in L.vrhip_last_error()
        assert L.vrhip_trace_surface(q._ctx, None, p(d), 64, p(out)) == -1
        assert L.vrhip_trace_surface(q._ctx, p(o), None, 64, p(out)) == -1
        assert L.vrhip_trace_surface(q._ctx, p(o), p(d), 64, None) == -1
        assert L.vrhip_camera_rays(q._ctx, None, p(out)) == -1 and L.vrhip_camera_rays(q._ctx, p(out), None) == -1
        assert L.vrhip_trace_surface(q._ctx, None, None, 0, None) == 0
        assert L.vrhip_trace_surface(q._ctx, p(o), p(d), 0, p(out)) == 0
        assert not out.cpu().numpy().any()               # nothing was written by any of them
        wrong = [dict(origins=o.cpu(), dirs=d), dict(origins=o, dirs=d.double()), dict(origins=o, dirs=d[:-1]),
                 dict(origins=o[:, :2].contiguous(), dirs=d), dict(origins=None, dirs=d), dict(origins=o, dirs=None)]
        for kw in wrong:                                 # device, dtype, shape, missing
            with pytest.raises(ValueError):
                q.traceSurface(**kw)
        again = q.traceSurface(o, d)["record"].cpu().numpy()
        assert (sf.u32(again) == sf.u32(want)).all()
    finally:
        q.cleanUp()
