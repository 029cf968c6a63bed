"""The BVH built on the GPU from device-resident triangles
(vrhip_upload_mesh_device): tree invariants on the exported tree, renders
bit-exact against the portable oracle walking that same tree, transactional
errors, replacement, and the builder's outward fp16 box rounding."""
import math

import numpy as np
import pytest

import pyoracle as po
from device_mesh_cases import (HARD_KINDS, bitexact, built_export, device_build, expected_triangles, fresh, hard_mesh,
                               loaded, sorted_rows, soup)
from half_ref import half_reference, half_values
from vrenderer_pathtracer_amd import (VRendererHIP, VRHIPError, build_flat, scenes, selftest_half_box,
                                      validate_flat)

pytestmark = pytest.mark.gpu

TERM = 0x80000000


# ---- the exported tree, analysed with numpy (vectorised per tree level) --------
def analyse(flat, mesh, max_leaf):
    """Checks every invariant of the issue on an exported tree; returns (depth, leaves)."""
    n_tris = len(mesh["tris"])
    n_refs = max(n_tris, 2)
    L = max(2, -(-n_refs // max_leaf))
    depth, n_nodes = validate_flat(flat)
    assert depth <= math.ceil(math.log2(L)) + 1, (depth, L)
    nodes = flat["bvh"].reshape(-1, 4, 4)
    assert len(nodes) == n_nodes == L - 1
    child = nodes[:, 3, :2].copy().view(np.int32)                        # (N, 2)
    verts = flat["verts"]
    is_term = verts[:, 0].copy().view(np.uint32) == TERM
    term_pos = np.flatnonzero(is_term)
    # leaves: runs of triples up to the next terminator, each with one parent
    leaf_mask = child < 0
    starts = np.sort(~child[leaf_mask])
    assert len(starts) == L and len(np.unique(starts)) == L
    ends = term_pos[np.searchsorted(term_pos, starts)]
    counts = (ends - starts) // 3
    assert ((ends - starts) % 3 == 0).all()
    assert counts.min() >= 1 and counts.max() <= max_leaf, (counts.min(), counts.max())
    assert counts.max() - counts.min() <= 1
    # the runs tile the slot arrays, so the non-terminator slots are the triangles
    assert starts[0] == 0 and (starts[1:] == ends[:-1] + 1).all() and ends[-1] == len(verts) - 1
    assert len(verts) == 3 * n_refs + L
    assert (verts[~is_term, 3] == 0).all()
    got = np.concatenate([verts[~is_term, :3], flat["normals"][~is_term, :3], flat["tangents"][~is_term, :3],
                          flat["uvs"][~is_term]], -1).reshape(n_refs, -1)
    assert np.array_equal(sorted_rows(got), sorted_rows(expected_triangles(mesh)))
    # exact boxes, bottom-up: leaf boxes from their vertices, inner boxes level by level
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
    return depth, L


# ---- 1. tree invariants -------------------------------------------------------
@pytest.mark.parametrize("max_leaf", [1, 2, 3])
@pytest.mark.parametrize("n_tris", [1, 2, 3, 5, 63, 64, 65, 257, 1000])
def test_tree_invariants(native, n_tris, max_leaf):
    mesh = soup(n_tris, seed=5)
    flat, info = built_export(mesh, max_leaf)
    depth, L = analyse(flat, mesh, max_leaf)
    assert info == (depth, L - 1, len(flat["verts"]))


# ---- 2. hard inputs -----------------------------------------------------------
@pytest.mark.parametrize("kind", HARD_KINDS)
def test_hard_inputs_valid_and_bitexact(native, oracle, kind):
    mesh = hard_mesh(kind)
    sc = scenes.make_scene("C2", 64, 48)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    device_build(r, mesh, 2)
    flat = r.export_mesh_flat()
    analyse(flat, mesh, 2)
    times = [4242, 4249]
    r.render(frames=2, times=times)
    ga, gr, gd = r.read_accum(), r.read_rgba8(), r.read_depth8()
    r.cleanUp()
    sc = dict(sc, mesh_flat=flat)
    oa, orgba, od, _ = po.render(sc, frames=2, times=times, libm=po.LIBM_PORTABLE)
    assert np.array_equal(ga.view(np.uint32), oa.view(np.uint32))
    assert np.array_equal(gr, orgba) and np.array_equal(gd, od)


# ---- 3. determinism -------------------------------------------------------------
def test_two_builds_are_byte_identical(native):
    mesh = scenes.torus_knot(60, 30)
    a, _ = built_export(mesh)
    b, _ = built_export(mesh)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- 4. mid size ----------------------------------------------------------------
def test_mid_size_knot(native):
    mesh = scenes.torus_knot(300, 150)                 # 90k triangles
    flat, info = built_export(mesh)
    depth, L = analyse(flat, mesh, 2)
    assert L == 45000 and depth <= 17 and info[0] == depth


# ---- 5. render parity -----------------------------------------------------------
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_render_parity_on_device_built_knot(native, oracle, name):
    mesh = scenes.torus_knot(100, 50)
    sc = scenes.make_scene(name, 160, 96)
    times = [12345 + 7 * i for i in range(3)]
    r = loaded(sc, mesh)
    sc = dict(sc, mesh_flat=r.export_mesh_flat())
    assert r.bvh_info()[0] == 13                      # ceil(log2 5000): 16-entry stacks
    r.render(frames=3, times=times)
    ga, gr, gd = r.read_accum(), r.read_rgba8(), r.read_depth8()
    oa, orgba, od, _ = po.render(sc, frames=3, times=times, libm=po.LIBM_PORTABLE)
    bitexact(ga, oa, f"{name} accum")
    bitexact(gr, orgba, f"{name} rgba8")
    bitexact(gd, od, f"{name} depth8")
    assert np.any(oa[..., :3] != 0)
    # every pierced box visited, as the reference walks: the same image
    r.set_strict_traversal(True)
    r.clearBuffer()
    r.render(frames=3, times=times)
    bitexact(r.read_accum(), ga, f"{name} strict traversal")
    r.cleanUp()
    if name == "C2":                                  # a render-service session: two unsynchronised 2-frame calls
        t4 = times + [99991]
        r = loaded(sc, mesh)
        r.set_service(1)
        r.render(frames=2, times=t4[:2], sync=False)
        r.render(frames=2, times=t4[2:], sync=False)
        r.sync()
        sa = r.read_accum()
        assert r.service_info()["served"] >= 1
        r.cleanUp()
        o4, _, _, _ = po.render(sc, frames=4, times=t4, libm=po.LIBM_PORTABLE)
        bitexact(sa, o4, "C2 service session")
    else:                                             # rank 0 of 2 renders the tiles it owns
        r = loaded(sc, mesh)
        r.set_tiling(0, 2)
        r.render(frames=3, times=times)
        ta = r.read_accum()
        r.cleanUp()
        tiles_x = sc["width"] // 16
        own = np.zeros(ta.shape[:2], bool)
        for t in range(0, tiles_x * (sc["height"] // 16), 2):
            ty = t // tiles_x
            tx = (t % tiles_x + ty) % tiles_x          # row-rotated dealing (include/vrhip.h)
            own[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = True
        assert (ta[own].view(np.uint32) == oa[own].view(np.uint32)).all()


# ---- 6. tree independence -------------------------------------------------------
def test_device_tree_equals_brute_force(native, oracle):
    mesh = soup(300, seed=5)
    mesh.update(normals=np.tile([0, 0, 1], (900, 1)).astype(np.float32),
                tangents=np.tile([1, 0, 0], (900, 1)).astype(np.float32))
    flat, _ = built_export(mesh, 3)
    sc = scenes.make_scene("C2", 48, 32)
    sc["mesh_flat"] = flat
    a, _, _, _ = po.render(sc, frames=1)
    b, _, _, _ = po.render(sc, frames=1, brute_force=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 7. the exporter alone -------------------------------------------------------
def test_export_returns_an_uploaded_flat_tree_byte_for_byte(native):
    flat = build_flat(scenes.torus_knot(40, 20))
    r = fresh()
    r.initMesh(flat)
    out = r.export_mesh_flat()
    r.cleanUp()
    for k in ("bvh", "verts", "normals", "tangents", "uvs"):
        assert out[k].shape == flat[k].shape and out[k].tobytes() == flat[k].tobytes(), k


def test_export_without_a_mesh_is_invalid(native):
    r = fresh()
    with pytest.raises(VRHIPError) as e:
        r.export_mesh_flat()
    assert e.value.code == -1
    r.cleanUp()


# ---- 8. errors are transactional ---------------------------------------------------
def test_errors_leave_the_resident_mesh(native):
    mesh = scenes.torus_knot(40, 20)
    sc = scenes.make_scene("C2", 64, 48)
    r = loaded(sc, mesh)
    r.render(frames=2, times=[1, 2])
    first = r.read_accum()
    info = r.bvh_info()
    nv = len(mesh["positions"])
    bad_index = dict(mesh, tris=mesh["tris"].copy())
    bad_index["tris"][777, 1] = nv
    nan_vertex = dict(mesh, positions=mesh["positions"].copy())
    nan_vertex["positions"][int(mesh["tris"][5, 2]), 1] = np.nan
    empty = dict(mesh, tris=np.zeros((0, 3), np.uint32))
    for bad, leaf in ((bad_index, 2), (nan_vertex, 2), (empty, 2), (mesh, 128)):
        with pytest.raises(VRHIPError) as e:
            device_build(r, bad, leaf)
        assert e.value.code == -1
    assert r.bvh_info() == info
    r.clearBuffer()
    r.render(frames=2, times=[1, 2])
    assert np.array_equal(r.read_accum().view(np.uint32), first.view(np.uint32))
    r.cleanUp()


def test_wrong_tensors_raise_value_error(native):
    import torch
    mesh = scenes.torus_knot(8, 6)
    r = fresh()
    pos = torch.from_numpy(mesh["positions"]).cuda(0)
    tri = torch.from_numpy(np.ascontiguousarray(mesh["tris"], np.int32)).cuda(0)
    with pytest.raises(ValueError):
        r.initMeshDevice(pos.cpu(), tri)
    with pytest.raises(ValueError):
        r.initMeshDevice(pos.double(), tri)
    with pytest.raises(ValueError):
        r.initMeshDevice(pos, tri.long())
    with pytest.raises(ValueError):
        r.initMeshDevice(pos.t().contiguous().t(), tri)
    with pytest.raises(ValueError):
        r.initMeshDevice(pos, tri, normals=pos[:-1])
    r.initMeshDevice(pos, tri)
    r.cleanUp()


def test_multi_device_context_is_refused(native):
    import torch
    mesh = scenes.torus_knot(8, 6)
    r = VRendererHIP([0])
    r.init(64, 48)
    with pytest.raises(VRHIPError) as e:
        r.initMeshDevice(torch.from_numpy(mesh["positions"]).cuda(0),
                         torch.from_numpy(np.ascontiguousarray(mesh["tris"], np.int32)).cuda(0))
    assert e.value.code == -1 and "multi-device" in str(e.value)
    r.cleanUp()


# ---- 9. replacement -------------------------------------------------------------
def test_replacing_a_device_mesh_between_unsynchronised_renders(native):
    a, b = scenes.torus_knot(40, 20), scenes.torus_knot(30, 12)
    sc = scenes.make_scene("C2", 64, 48)
    r = loaded(sc, a)
    r.set_service(1)
    r.render(frames=2, times=[1, 2], sync=False)
    s0 = r.service_info()["sessions"]
    device_build(r, b, 2)
    r.clearBuffer()
    r.render(frames=2, times=[3, 4], sync=False)
    r.sync()
    got = r.read_accum()
    si = r.service_info()
    assert si["sessions"] > s0 >= 1 and si["refused"] == 0
    r.cleanUp()
    r = loaded(sc, b)
    r.set_service(1)
    r.render(frames=2, times=[3, 4])
    assert np.array_equal(got.view(np.uint32), r.read_accum().view(np.uint32))
    r.cleanUp()


# ---- 10. half boxes ---------------------------------------------------------------
def test_half_box_rounding_matches_numpy_reference(native):
    x = half_values()
    down, up = selftest_half_box(x)
    assert np.array_equal(down, half_reference(x, False))
    assert np.array_equal(up, half_reference(x, True))
    with np.errstate(over="ignore"):
        assert (down.view(np.float16).astype(np.float32) <= x).all()
        assert (up.view(np.float16).astype(np.float32) >= x).all()
