"""Surface records without a ray: at points of the resident mesh
(vrhip_surface_at) and at the texels of a lightmap atlas of its uvs
(vrhip_atlas_surface, vr_atlas.hip).

The yardstick is tests/atlas_cases.py (the oracle's own leaf_hit and the
definition of include/vrhip.h restated in plain C; pinned in
test_atlas_cpu.py): all 28 words of every record equal it, compared as uint32.
Only where the mesh has zero tangents, and the record's tangent is therefore
normalize(0), a float word may instead be NaN on both sides, as in the surface
query's tests.  Then the product against itself: surfaceAt against
traceSurface, the atlas through surfaceAt, the bake loop closed through a
render's own map fetch, and atlas -> shadeSurface -> denoise end to end."""
import ctypes

import numpy as np
import pytest

import atlas_cases as ac
import surface_cases as sf
from device_mesh_cases import deform, device_build, fresh
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, scenes

pytestmark = pytest.mark.gpu


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda(0)


@pytest.fixture(scope="module", autouse=True)
def _built(native, oracle):
    yield


def loaded(sc):
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    return r


def words(out, n):
    """The [n, 28] records as uint32, the dict's views checked against them."""
    import torch
    rec = out["record"]
    assert rec.is_cuda and tuple(rec.shape) == (n, 28) and rec.dtype == torch.float32
    assert set(out) == {"record", "t", "kind", "prim", "type", "position", "normal", "tangent", "color", "specular",
                        "emission", "bary", "uv"}
    assert out["prim"].data_ptr() == rec[:, sf.PRIM].data_ptr() and out["prim"].dtype == torch.int32
    assert out["bary"].data_ptr() == rec[:, sf.BARY_U].data_ptr() and out["bary"].stride() == (28, 4)
    assert out["uv"].data_ptr() == rec[:, sf.TEX_U].data_ptr() and tuple(out["color"].shape) == (n, 3)
    return np.ascontiguousarray(rec.cpu().numpy()).view(np.uint32)


def atlas(r, w, h, gutter=0):
    return words(r.atlasRecords(w, h, gutter), w * h)


def check(r, sc, w, h, gutter, what, box=False, nan_ok=False, prim_of_slot=None):
    want = ac.raster(sc, w, h, gutter, box=box, prim_of_slot=prim_of_slot)
    got = atlas(r, w, h, gutter)
    ac.same(got, want, f"{what} {w}x{h} gutter {gutter}", nan_ok)
    return got, want


# ---- 1. texel-centre ties -------------------------------------------------------------------------------
@pytest.mark.parametrize("mirrored", [False, True], ids=["ccw", "mirrored"])
@pytest.mark.parametrize("swap_order", [False, True], ids=["order01", "order10"])
def test_centres_on_a_shared_edge_go_to_the_lower_prim(swap_order, mirrored):
    flat = ac.flat_of("quad", swap_order, mirrored)
    sc = ac.scene_of(flat)
    r = loaded(sc)
    try:
        got, _ = check(r, sc, 8, 8, 0, "quad")
        g = got.reshape(8, 8, 28)
        assert (g[..., sf.KIND] == sf.MESH).all()
        assert (g[np.arange(8), np.arange(8), sf.PRIM] == ac.first_slots(flat).min()).all()
        mesh = ac.quad(swap_order, mirrored)            # the same through a device build: prim is the row of tris
        device_build(r, mesh, 2, "morton")
        ex = r.export_mesh_flat()
        got, _ = check(r, dict(sc, mesh_flat=ex), 8, 8, 0, "quad, device build", prim_of_slot=ac.prim_of_slot(ex, mesh))
        assert not got.reshape(8, 8, 28)[np.arange(8), np.arange(8), sf.PRIM].any()
    finally:
        r.cleanUp()


# ---- 2. mesh shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["host", "morton", "sah"])
def test_the_single_triangle_mesh(builder):
    """Stored twice, under two leaves."""
    mesh = ac.single_triangle()
    flat = ac.flat_of("single_triangle")
    assert len(ac.first_slots(flat)) == 2
    sc = ac.scene_of(flat, "maps_odd")
    r = loaded(sc)
    try:
        pos = None
        if builder != "host":
            device_build(r, mesh, 2, builder)
            flat = r.export_mesh_flat()
            sc, pos = dict(sc, mesh_flat=flat), ac.prim_of_slot(flat, mesh)
        for w, h, g in ((7, 5, 0), (33, 31, 2)):
            got, _ = check(r, sc, w, h, g, f"one triangle, {builder}", prim_of_slot=pos)
            assert (got[:, sf.KIND] == sf.MESH).any() and (got[:, sf.KIND] == sf.NONE).any()
        prims = np.unique(got[got[:, sf.KIND] == sf.MESH, sf.PRIM])
        assert prims.tolist() == [0 if pos is not None else int(ac.first_slots(flat).min())]
    finally:
        r.cleanUp()


def test_a_mesh_without_uvs_is_all_misses():
    mesh = ac.knot(0.0, uvs=False)
    r = loaded(ac.scene_of(None))
    try:
        device_build(r, mesh, 2, "morton")
        got = atlas(r, 33, 17, 3)
        want = np.zeros((33 * 17, 28), np.uint32)
        want[:, sf.T], want[:, sf.PRIM] = sf.u32(sf.NO_HIT), sf.MISS
        ac.same(got, want, "no uvs")
        sc = ac.scene_of(ac.flat_of("knot", 0.0, False))
        assert (ac.raster(sc, 33, 17, 3) == want).all()
    finally:
        r.cleanUp()


# ---- 3. atlas shapes --------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 64), (64, 1), (7, 5), (65, 63), (300, 200)]


@pytest.fixture(scope="module")
def knots():
    live = {}
    for margin in (0.0, 0.1):
        sc = ac.scene_of(ac.flat_of("knot", margin), "maps_odd")
        live[margin] = (loaded(sc), sc)
    yield live
    for r, _ in live.values():
        r.cleanUp()


@pytest.mark.parametrize("margin", [0.0, 0.1])
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_atlas_shapes(knots, w, h, margin):
    r, sc = knots[margin]
    got, _ = check(r, sc, w, h, 0, f"knot margin {margin}", box=w * h > 10000)
    covered = (got[:, sf.KIND] == sf.MESH).mean()
    if margin == 0.0:
        assert covered == 1.0
    elif w * h >= 35:
        assert 0.4 < covered < 0.85            # the chart's share is 0.64; a 64 x 1 strip sees 52 of 64
    check(r, sc, w, h, 1, f"knot margin {margin}", box=w * h > 10000)


# ---- 4. big against small ---------------------------------------------------------------------------------
@pytest.mark.parametrize("big_first", [True, False], ids=["big_wins", "big_loses"])
def test_big_against_small(big_first):
    flat = ac.flat_of("big_small", big_first)
    sc = ac.scene_of(flat, "maps_tall")
    r = loaded(sc)
    try:
        got, _ = check(r, sc, 300, 200, 0, "big and small", box=True)
        assert len(ac.first_slots(flat)) == 502 and (got[:, sf.KIND] == sf.MESH).all()
        # (after a host upload the winner is the lowest flat slot, and build_flat keeps no caller order)
        mesh = ac.big_small(big_first)
        device_build(r, mesh, 2, "sah")                             # here the caller's order decides
        ex = r.export_mesh_flat()
        got, _ = check(r, dict(sc, mesh_flat=ex), 300, 200, 0, "big and small, device", box=True,
                       prim_of_slot=ac.prim_of_slot(ex, mesh))
        if big_first:
            assert (got[:, sf.PRIM] < 2).all()
        else:
            small = got[:, sf.PRIM] < 500
            assert small.sum() > 100 and (got[~small, sf.PRIM] >= 500).all()
    finally:
        r.cleanUp()


# ---- 5. hostile uvs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(65, 63), (1, 1), (300, 7)])
def test_hostile_uvs(w, h):
    flat = ac.flat_of("hostile")
    sc = ac.scene_of(flat, "maps_odd")
    r = loaded(sc)
    try:
        got, _ = check(r, sc, w, h, 0, "hostile")
        check(r, sc, w, h, 2, "hostile")
        if w * h > 1:
            # the triangles with a vertex at +-1e9 or +-3e38 cover whatever the others leave: no miss, many winners
            assert (got[:, sf.KIND] == sf.MESH).all() and len(np.unique(got[:, sf.PRIM])) >= 8
        mesh = ac.hostile()
        device_build(r, mesh, 2, "morton")
        ex = r.export_mesh_flat()
        check(r, dict(sc, mesh_flat=ex), w, h, 1, "hostile, device", prim_of_slot=ac.prim_of_slot(ex, mesh))
    finally:
        r.cleanUp()


# ---- 6. gutter ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def charts():
    sc = ac.scene_of(ac.flat_of("chart_mesh"), "plain", 96, 64)
    r = loaded(sc)
    yield r, sc
    r.cleanUp()


@pytest.mark.parametrize("gutter", [0, 1, 2, 8, 64])
def test_gutter(charts, gutter):
    r, sc = charts
    w, h = ac.CHART_W, ac.CHART_H
    got, _ = check(r, sc, w, h, gutter, "charts")
    t = sf.floats(got)[:, sf.T]
    hit = got[:, sf.KIND] == sf.MESH
    # t is the pass that reached the texel: every pass up to the last one that found work reached some
    assert set(np.unique(t[hit]).tolist()) == set(float(k) for k in range(int(t[hit].max()) + 1))
    assert t[hit].max() <= gutter and (t[~hit] == sf.NO_HIT).all()
    if gutter <= 8:
        assert t[hit].max() == gutter and (~hit).any()
    else:
        assert hit.all()                                # every texel of 65 x 63 lies within 64 of a chart
    if gutter in (1, 2):
        prev = atlas(r, w, h, gutter - 1)               # a pass only adds texels, next to covered ones
        was = prev[:, sf.KIND] == sf.MESH
        assert (got[was] == prev[was]).all() and (hit & ~was).any()
        grid = was.reshape(h, w)
        near = np.zeros_like(grid)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                near[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] |= grid[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
        assert ((hit & ~was).reshape(h, w) == (near & ~grid)).all()


# ---- 7. scenes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ac.SCENE_KINDS)
def test_scenes(kind):
    sc = ac.scene_of(ac.flat_of("knot", 0.1), kind)
    r = loaded(sc)
    try:
        got, want = check(r, sc, 65, 63, 1, kind, nan_ok=kind == "tan0")
        hit = got[:, sf.KIND] == sf.MESH
        assert (got[hit, sf.TYPE] == (2 if kind == "brdf_view" else 1)).all()
        f = sf.floats(got)[hit]
        if kind == "tan0":
            assert np.isnan(f[:, sf.TANGENT]).all()
        if kind in ("maps_odd", "maps_tall"):
            assert len(np.unique(got[hit][:, sf.COLOR], axis=0)) > 20 and (f[:, sf.SPECULAR] != 0).any()
        if kind in ("plain", "brdf_view"):
            assert (f[:, sf.COLOR] == 1.0).all() and not got[hit][:, sf.SPECULAR].any()
        for cornell, example in ((True, False), (False, True), (True, True), (False, False)):
            r.useCornellBox(cornell)
            r.useExampleSphere(example)
            ac.same(atlas(r, 65, 63, 1), got, f"{kind} cornell={cornell} example={example}")
    finally:
        r.cleanUp()


# ---- 8. independence from the tree --------------------------------------------------------------------------
def test_the_tree_does_not_matter():
    """64 x 48: no texel centre lies on an edge of the 24 x 12 knot's chart
    (3 (2x + 1) = 16 i and 2y + 1 = 8 j have no solutions, nor has the
    diagonal's 3 (2x + 1) - 2 (2y + 1) = 16 k), so the winner does not depend on
    how the caller's triangles are numbered either."""
    import torch
    mesh = ac.knot(0.0)
    w, h = 64, 48
    sc = ac.scene_of(None, "maps_odd")
    tri_rows = {}
    r = loaded(sc)
    try:
        for builder in ("morton", "sah", "host"):
            if builder == "host":
                r.initMesh(mesh)
            else:
                device_build(r, mesh, 2, builder)
            ex = r.export_mesh_flat()
            rows = ac.prim_of_slot(ex, mesh)
            got, _ = check(r, dict(sc, mesh_flat=ex), w, h, 2, builder, prim_of_slot=None if builder == "host" else rows)
            assert (got[:, sf.KIND] == sf.MESH).all()
            if builder == "host":
                got = got.copy()
                got[:, sf.PRIM] = rows[got[:, sf.PRIM]]             # the flat slot back to the row of tris
            tri_rows[builder] = got
        ac.same(tri_rows["sah"], tri_rows["morton"], "sah against morton")
        ac.same(tri_rows["host"], tri_rows["morton"], "host against morton")
        # a refit: the same triangles at the same texels, the whole record the yardstick's on the deformed mesh
        device_build(r, mesh, 2, "morton")
        before = atlas(r, w, h, 2)
        moved = deform(mesh["positions"])
        r.refitMeshDevice(dev(moved))
        ex = r.export_mesh_flat()
        moved_mesh = dict(mesh, positions=moved)
        after, _ = check(r, dict(sc, mesh_flat=ex), w, h, 2, "refit", prim_of_slot=ac.prim_of_slot(ex, moved_mesh))
        keep = [sf.T, sf.KIND, sf.PRIM, sf.TYPE, sf.BARY_U, sf.BARY_V, sf.TEX_U, sf.TEX_V, sf.PAD0, sf.PAD1]
        keep += list(range(16, 19)) + list(range(20, 23)) + list(range(24, 27))       # color, specular, emission
        assert (after[:, keep] == before[:, keep]).all()
        assert (after[:, sf.POSITION] != before[:, sf.POSITION]).any()
        p = r.surfaceAt(torch.from_numpy(after[:, sf.PRIM].astype(np.int32)).cuda(0), dev(sf.floats(after)[:, [sf.BARY_U, sf.BARY_V]]))
        ac.same(words(p, w * h)[:, 1:], after[:, 1:], "surfaceAt after the refit (the inverse map is kept)")
    finally:
        r.cleanUp()


# ---- 9. surfaceAt -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("name", ["cornell+mesh", "mesh+tex_d+tex_n+tex_s", "cornell+view_brdf+mesh+brdf+tex_d+tex_s"])
def test_surface_at_is_trace_surface_without_the_ray(name, strict):
    import torch
    sc = sf.scene_named(name)
    r = loaded(sc)
    r.set_strict_traversal(strict)
    cols = np.ones(28, bool)
    cols[sf.T] = False
    cols[sf.POSITION] = False
    try:
        n_mesh = 0
        for which in ("A", "B"):
            o, d = (r.cameraRays() if which == "A" else tuple(dev(a) for a in sf.ray_set("B")))
            hits = words(r.traceSurface(o, d), len(o))
            m = hits[:, sf.KIND] == sf.MESH
            n_mesh += int(m.sum())
            prims = torch.from_numpy(hits[:, sf.PRIM].astype(np.int64)).cuda(0)
            prims[~torch.from_numpy(m).cuda(0)] = -1                  # a sphere's index names a triangle too: ask for none
            got = words(r.surfaceAt(prims, dev(sf.floats(hits)[:, [sf.BARY_U, sf.BARY_V]])), len(o))
            ac.same(got[m][:, cols], hits[m][:, cols], f"{name} set {which}")
            assert not got[m][:, sf.T].any() and not got[~m].any()
            if which == "B":                                          # and the yardstick, every word of its finite records
                want = ac.at(sc, hits[m, sf.PRIM], sf.floats(hits[m])[:, [sf.BARY_U, sf.BARY_V]])
                fin = sf.kept(want)
                ac.same(got[m][fin], want[fin], f"{name} yardstick")
        assert n_mesh >= 50
    finally:
        r.cleanUp()


def test_surface_at_of_the_atlas_is_the_atlas(knots):
    import torch
    r, sc = knots[0.1]
    w, h = 65, 63
    rec = atlas(r, w, h, 2)
    out = r.surfaceAt(torch.from_numpy(rec[:, sf.PRIM].view(np.int32).copy()).cuda(0), dev(sf.floats(rec)[:, [sf.BARY_U, sf.BARY_V]]))
    got = words(out, w * h)
    hit = rec[:, sf.KIND] == sf.MESH
    ac.same(got[hit][:, 1:], rec[hit][:, 1:], "surfaceAt of the atlas")
    assert not got[hit][:, sf.T].any() and not got[~hit].any() and hit.any() and (~hit).any()


def test_surface_at_invalid_and_extrapolating_entries(knots):
    import torch
    r, sc = knots[0.1]
    flat = sc["mesh_flat"]
    slots = ac.first_slots(flat)
    n_slots = len(np.asarray(flat["verts"]).reshape(-1, 4))
    rng = np.random.default_rng(9)
    good = slots[rng.integers(0, len(slots), 64)]
    bary = rng.uniform(0.0, 0.5, (64, 2)).astype(np.float32)
    prims = good.astype(np.uint32).copy()
    bad = np.arange(0, 64, 4)
    bary[1] = (2.0, -1.0)                                    # extrapolation is the caller's business
    bary[2] = (-0.5, 3.0)
    bary[3] = (1e3, 1e3)
    for k, i in enumerate(bad):
        if k % 6 == 0:
            prims[i] = n_slots + k                           # past the mesh
        elif k % 6 == 1:
            prims[i] = good[i] + 1                           # a slot that is not a first vertex
        elif k % 6 == 2:
            prims[i] = sf.MISS
        elif k % 6 == 3:
            bary[i, 0] = np.nan
        elif k % 6 == 4:
            bary[i, 1] = np.inf
        else:
            bary[i] = (-np.inf, np.nan)
    want = ac.at(sc, prims, bary)
    assert not want[bad].any() and want[np.setdiff1d(np.arange(64), bad)].any(-1).all()
    got = words(r.surfaceAt(torch.from_numpy(prims.view(np.int32)).cuda(0), dev(bary)), 64)
    ac.same(got, want, "invalid and extrapolating entries")
    # one past the last triangle after a device build; canary rows past n stay
    mesh = ac.knot(0.1)
    q = fresh()
    try:
        device_build(q, mesh, 2, "morton")
        n_tris = len(mesh["tris"])
        p = torch.tensor([0, n_tris - 1, n_tris, -1], dtype=torch.int32, device="cuda:0")
        b = torch.full((4, 2), 0.25, dtype=torch.float32, device="cuda:0")
        out = torch.full((6, 28), -7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        vp = lambda x: ctypes.c_void_p(x.data_ptr())                            # noqa: E731
        assert q._lib.vrhip_surface_at(q._ctx, vp(p), vp(b), 4, vp(out)) == 0
        got = np.ascontiguousarray(out.cpu().numpy()).view(np.uint32)
        assert (got[4:] == sf.u32(np.float32(-7.0))).all() and not got[2:4].any()
        assert (got[:2, sf.KIND] == sf.MESH).all() and got[0, sf.PRIM] == 0 and got[1, sf.PRIM] == n_tris - 1
    finally:
        q.cleanUp()


# ---- 10. the loop closes ----------------------------------------------------------------------------------
def test_a_render_fetches_the_texel_the_atlas_filled():
    sc = ac.scene_of(ac.flat_of("chart_mesh"), "plain", 96, 64)
    r = loaded(sc)
    w, h = ac.CHART_W, ac.CHART_H
    rec = atlas(r, w, h, 1)
    covered = rec[:, sf.KIND] == sf.MESH
    tex = np.zeros((h, w, 4), np.float32)
    tex[..., 0] = np.arange(w * h, dtype=np.float32).reshape(h, w)
    tex[..., 1] = covered.reshape(h, w)
    r.loadTexture(tex, 1.0, 0)
    try:
        o, d = r.cameraRays()
        hits = words(r.traceSurface(o, d), len(o))
        m = hits[:, sf.KIND] == sf.MESH
        assert m.sum() >= 300
        f = sf.floats(hits)[m]
        want = ac.tex_addr(w, h, f[:, sf.TEX_U], f[:, sf.TEX_V])
        assert (f[:, 16] == want.astype(np.float32)).all()
        assert (f[:, 17] == 1.0).all(), "a hit fetched a texel the atlas left empty"
        assert len(np.unique(want)) >= 200
    finally:
        r.cleanUp()


# ---- 11. end to end -----------------------------------------------------------------------------------------
def test_atlas_shade_denoise(knots):
    import torch
    r, sc = knots[0.1]
    w, h = 65, 63
    want_rec = ac.raster(sc, w, h, 1)
    rng = np.random.default_rng(10)
    seeds = torch.from_numpy(rng.integers(0, 2**31, (w * h, 2), dtype=np.int64).astype(np.int32)).cuda(0)
    outs = []
    for rec in (r.atlasRecords(w, h, 1)["record"], torch.from_numpy(want_rec.view(np.float32)).cuda(0)):
        dirs = -rec[:, 8:11].contiguous()                    # against the normal; a miss has none: (0, 0, 0), an invalid direction
        rad = r.shadeSurface(rec, dirs, seeds, samples=4)
        out = r.denoise(rad.view(h, w, 4), rec)
        outs.append((rad.cpu().numpy().view(np.uint32), out.cpu().numpy().view(np.uint32).reshape(-1, 4)))
    assert (outs[0][0] == outs[1][0]).all() and (outs[0][1] == outs[1][1]).all()
    miss = want_rec[:, sf.KIND] == sf.NONE
    assert miss.any() and not outs[0][1][miss].any()
    lit = outs[0][1][~miss].view(np.float32)[:, :3]
    assert np.isfinite(lit).all() and (lit > 0).any(-1).mean() > 0.9
    assert (outs[0][0][~miss] != outs[0][1][~miss]).any(), "the filter changed nothing"


# ---- 12. errors and state -----------------------------------------------------------------------------------
def test_refusals():
    import torch
    vp = lambda x: ctypes.c_void_p(x.data_ptr())                                # noqa: E731
    out = torch.zeros((65, 28), dtype=torch.float32, device="cuda:0")
    prims = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    bary = torch.zeros((8, 2), dtype=torch.float32, device="cuda:0")
    q = VRendererHIP([0])                                    # a multi-device context of one device
    q.init(64, 48)
    q.initMesh(ac.flat_of("knot", 0.1))
    for fn in (lambda: q.atlasRecords(8, 8), lambda: q.surfaceAt(prims, bary)):
        with pytest.raises(VRHIPError) as e:
            fn()
        assert e.value.code == -1 and "multi-device" in str(e.value)
    q.cleanUp()
    q = fresh()
    try:
        L = q._lib
        torch.cuda.synchronize()
        assert L.vrhip_atlas_surface(q._ctx, 8, 8, 0, vp(out)) == -1 and b"no mesh" in L.vrhip_last_error()
        assert L.vrhip_surface_at(q._ctx, vp(prims), vp(bary), 8, vp(out)) == -1 and b"no mesh" in L.vrhip_last_error()
        with pytest.raises(VRHIPError):
            q.atlasRecords(8, 8)
        q.initMesh(ac.flat_of("knot", 0.1))                  # HDRI mode, no environment map: none is needed
        assert L.vrhip_atlas_surface(q._ctx, 8, 8, 0, vp(out)) == 0
        ok = out.cpu().numpy().copy()
        assert ok[:64].any() and not ok[64:].any()
        for w, h, g in ((0, 8, 0), (8, 0, 0), (16385, 1, 0), (1, 16385, 0), (16384, 8192, 0), (8, 8, 65), (8, 8, 2**31)):
            assert L.vrhip_atlas_surface(q._ctx, w, h, g, vp(out)) == -1, (w, h, g)
        assert L.vrhip_atlas_surface(q._ctx, 8, 8, 0, None) == -1
        assert L.vrhip_atlas_surface(q._ctx, 8, 8, 0, ctypes.c_void_p(out.data_ptr() + 4)) == -1
        assert b"16-byte" in L.vrhip_last_error()
        assert L.vrhip_surface_at(q._ctx, None, vp(bary), 8, vp(out)) == -1
        assert L.vrhip_surface_at(q._ctx, vp(prims), None, 8, vp(out)) == -1
        assert L.vrhip_surface_at(q._ctx, vp(prims), vp(bary), 8, None) == -1
        assert L.vrhip_surface_at(q._ctx, vp(prims), vp(bary), 8, ctypes.c_void_p(out.data_ptr() + 8)) == -1
        assert L.vrhip_surface_at(q._ctx, None, None, 0, None) == 0
        assert (out.cpu().numpy().view(np.uint32) == ok.view(np.uint32)).all()       # none of them wrote
        for kw in (dict(width=0, height=8), dict(width=8, height=8, gutter=65), dict(width=16384, height=8192)):
            with pytest.raises(VRHIPError) as e:
                q.atlasRecords(**kw)
            assert e.value.code == -1
        with pytest.raises(ValueError):
            q.atlasRecords(8.5, 8)
        wrong = [dict(prims=prims.cpu(), bary=bary), dict(prims=prims.float(), bary=bary), dict(prims=prims, bary=bary[:-1]),
                 dict(prims=prims, bary=bary.double()), dict(prims=None, bary=bary), dict(prims=prims, bary=None),
                 dict(prims=prims.view(4, 2), bary=bary)]
        for kw in wrong:
            with pytest.raises(ValueError):
                q.surfaceAt(**kw)
        assert tuple(q.surfaceAt(prims[:0], bary[:0])["record"].shape) == (0, 28)
    finally:
        q.cleanUp()


@pytest.mark.parametrize("call", ["atlasRecords", "surfaceAt"])
def test_between_unsynchronised_renders_of_a_session(call):
    import torch
    sc = sf.scene_named("cornell+mesh")
    prims = torch.from_numpy(ac.first_slots(sc["mesh_flat"])[:64].astype(np.int32)).cuda(0)
    bary = torch.full((64, 2), 0.3, dtype=torch.float32, device="cuda:0")
    images = {}
    for query in (False, True):
        q = loaded(sc)
        q.set_service(1)
        q.render(frames=2, times=[11, 12], sync=False)
        if query:
            s0 = q.service_info()["sessions"]
            if call == "atlasRecords":
                ac.same(atlas(q, 33, 31, 1), ac.raster(sc, 33, 31, 1), "inside a session")
            else:
                ac.same(words(q.surfaceAt(prims, bary), 64), ac.at(sc, prims.cpu().numpy(), bary.cpu().numpy()), "inside a session")
        q.render(frames=2, times=[13, 14], sync=False)
        q.sync()
        if query:
            assert q.service_info()["sessions"] > s0 >= 1        # the call closed the first session
        assert q.getFrameCount() == 4
        images[query] = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.export_mesh_flat())
        q.cleanUp()
    for a, b in zip(images[False][:3], images[True][:3]):
        assert a.tobytes() == b.tobytes()
    assert all(images[False][3][k].tobytes() == images[True][3][k].tobytes() for k in images[True][3])
    assert np.any(images[True][0][..., :3] != 0)
