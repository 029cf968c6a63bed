"""The atlas yardstick without a device (tests/atlas_cases.py, atlas_driver.c;
vrhip_surface_at, vrhip_atlas_surface).

The yardstick is pinned to what is already pinned: on the mesh hits of the
surface query's ray sets, atlas_at(prim, bary_u, bary_v) is the record of the
oracle's intersect_scene in every word but t and position.  Its two rasters
agree.  The premise of the bake loop -- the texel the renderer's tex_addr
fetches for a point of a chart holds a record once one gutter pass has run --
is checked on the yardstick alone.  Then the mesh of scenes.torus_knot_unwrapped,
and what the C ABI refuses before any device call."""
import ctypes

import numpy as np
import pytest

import atlas_cases as ac
import surface_cases as sf

PINNED = ("cornell+mesh", "mesh+tex_d+tex_n+tex_s", "cornell+view_brdf+mesh+brdf+tex_d+tex_s")   # plain, every map, BRDF view


@pytest.mark.parametrize("name", PINNED)
def test_atlas_at_is_the_oracle_s_mesh_hit(oracle, native, name):
    """Every word but t and position bit for bit.  The barycentric position
    against the hit point o + d * t only loosely: observed on these sets at most
    4.3e-4 world units (the mesh spans about 80 and a ray travels up to 200;
    the triangle test's t and barycentrics each carry a few fp32 roundings),
    printed below; the bound asserted, 1e-2, only says that the two are the
    same point."""
    sc = sf.scene_named(name)
    n_mesh, worst = 0, 0.0
    for which in sf.sets_of(sc):
        rec, ok = sf.reference(name, which)
        m = (rec[:, sf.KIND] == sf.MESH) & ok
        n_mesh += int(m.sum())
        hits = rec[m]
        got = ac.at(sc, hits[:, sf.PRIM], sf.floats(hits)[:, [sf.BARY_U, sf.BARY_V]])
        cols = np.ones(28, bool)
        cols[sf.T] = False
        cols[sf.POSITION] = False
        ac.same(got[:, cols], hits[:, cols], f"{name} set {which}")
        assert not got[:, sf.T].any()
        if len(hits):
            d = np.abs(sf.floats(got)[:, sf.POSITION].astype(np.float64) - sf.floats(hits)[:, sf.POSITION].astype(np.float64))
            worst = max(worst, float(d.max()))
    print(f"{name}: {n_mesh} mesh hits, barycentric position within {worst:.3g} of the hit point")
    assert n_mesh >= 400 and worst < 1e-2


SMALL = [("quad", (), 8, 8), ("quad", (True, True), 8, 8), ("single_triangle", (), 7, 5), ("knot", (0.1,), 65, 63),
         ("knot", (0.0,), 7, 5), ("hostile", (), 65, 63), ("chart_mesh", (), ac.CHART_W, ac.CHART_H),
         ("big_small", (False, 60, 40, 100), 60, 40)]


@pytest.mark.parametrize("which,args,w,h", SMALL, ids=[f"{c[0]}{i}" for i, c in enumerate(SMALL)])
def test_the_two_rasters_agree(oracle, which, args, w, h):
    sc = ac.scene_of(ac.flat_of(which, *args))
    for gutter in (0, 2):
        brute = ac.raster(sc, w, h, gutter)
        ac.same(ac.raster(sc, w, h, gutter, box=True), brute, f"{which} {w}x{h} gutter {gutter}")
    covered = brute[:, sf.KIND] == sf.MESH
    assert covered.any() and ((brute[~covered, sf.KIND] == sf.NONE) & (brute[~covered, sf.PRIM] == ac.MISS)).all()


def test_quad_ties_go_to_the_lower_prim(oracle):
    for args in ((False, False), (True, False), (False, True), (True, True)):
        flat = ac.flat_of("quad", *args)
        rec = ac.raster(ac.scene_of(flat), 8, 8).reshape(8, 8, 28)
        assert (rec[..., sf.KIND] == sf.MESH).all()
        assert (rec[np.arange(8), np.arange(8), sf.PRIM] == ac.first_slots(flat).min()).all(), args


def test_the_texel_a_render_fetches_holds_a_record_after_one_gutter_pass(oracle):
    """The charts are axis-aligned rectangles at least one texel wide, so the
    centre of the texel that contains a point of a chart, or that of one of its
    8 neighbours, lies inside the chart."""
    sc = ac.scene_of(ac.flat_of("chart_mesh"))
    w, h = ac.CHART_W, ac.CHART_H
    _, u, v = ac.chart_points()
    texel = ac.tex_addr(w, h, u, v)
    assert (texel == np.floor(u.astype(np.float64) * w) + np.floor(v.astype(np.float64) * h) * w).all()
    with_gutter = ac.raster(sc, w, h, 1)
    without = ac.raster(sc, w, h, 0)
    assert (with_gutter[texel, sf.KIND] == sf.MESH).all()
    missed = int((without[texel, sf.KIND] == sf.NONE).sum())
    assert missed >= 1, "without a gutter some fetched texel must be a miss, or this test shows nothing"
    t = sf.floats(with_gutter)[:, sf.T]
    assert set(np.unique(t[with_gutter[:, sf.KIND] == sf.MESH]).tolist()) == {0.0, 1.0}


def test_the_unwrapped_knot():
    from vrenderer_pathtracer_amd import scenes
    nu, nv = 24, 12
    base = scenes.torus_knot(nu, nv)
    for margin in (0.0, 0.1):
        m = scenes.torus_knot_unwrapped(nu, nv, margin)
        assert len(m["positions"]) == (nu + 1) * (nv + 1) and len(m["tris"]) == 2 * nu * nv
        assert m["uvs"].dtype == np.float32 and m["tris"].dtype == np.uint32
        for key in ("positions", "normals", "tangents"):            # the same tube, triangle by triangle
            assert (m[key][m["tris"]] == base[key][base["tris"]]).all()
        uv = m["uvs"][m["tris"]].astype(np.float64)
        assert uv.min() >= margin - 1e-7 and uv.max() <= 1.0 - margin + 1e-7
        span = uv.max(1) - uv.min(1)
        assert (span[:, 0] < 1.01 / nu).all() and (span[:, 1] < 1.01 / nv).all(), "no triangle wraps"
        e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
        area = 0.5 * np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]).sum()
        assert abs(area - (1.0 - 2.0 * margin) ** 2) < 1e-5, "the chart fills [margin, 1 - margin]^2 once"
    assert (scenes.torus_knot(nu, nv)["uvs"] == base["uvs"]).all()


def test_symbols_are_exported(native):
    assert hasattr(native, "vrhip_surface_at") and hasattr(native, "vrhip_atlas_surface")


def test_c_abi_refuses_without_a_device(native):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert native.vrhip_surface_at(None, p, p, 1, p) == -1
    assert b"null ctx" in native.vrhip_last_error()
    assert native.vrhip_atlas_surface(None, 4, 4, 0, p) == -1
    assert b"null ctx" in native.vrhip_last_error()


def test_wrapper_has_the_methods(native):
    from vrenderer_pathtracer_amd import VRendererHIP
    assert callable(VRendererHIP.surfaceAt) and callable(VRendererHIP.atlasRecords)
    assert callable(VRendererHIP._surface_dict)
