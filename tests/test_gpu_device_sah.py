"""The host's binned-SAH tree built on the GPU from device-resident triangles
(vrhip_upload_mesh_device_ex, VRHIP_DEVBVH_SAH): the exported node array equals
vrhip_build_flat's byte for byte, leaves hold the host's triangles in ascending
input index, renders are bit-exact against the portable oracle walking the
exported tree, errors are transactional, and the Morton builder is unchanged."""
import numpy as np
import pytest

import device_mesh_cases as cases
import pyoracle as po
from device_mesh_cases import HARD_KINDS, bitexact, expected_triangles, hard_mesh, soup
from extreme_cases import check_boxes_and_leaves, slot_rows
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, build_flat, scenes, validate_flat

pytestmark = pytest.mark.gpu

T = 64                                                 # kSahSmall (csrc/vr_devsah.hpp): one wave64 per node up to here


# ---- builds: this file's default builder is the SAH one ---------------------------
def device_build(r, mesh, max_leaf=2, builder="sah", **kw):
    cases.device_build(r, mesh, max_leaf, builder, **kw)


def built_export(mesh, max_leaf=2, builder="sah"):
    return cases.built_export(mesh, max_leaf, builder)


def loaded(sc, mesh, builder="sah"):
    return cases.loaded(sc, mesh, builder)


_HOST = {}


def host_flat(key, mesh, max_leaf):
    """vrhip_build_flat's tree, built once per (mesh, max_leaf) and left unchanged."""
    if (key, max_leaf) not in _HOST:
        _HOST[(key, max_leaf)] = build_flat(mesh, max_leaf_tris=max_leaf)
    return _HOST[(key, max_leaf)]


# ---- the exported tree ---------------------------------------------------------
def leaf_of_triple(is_term):
    """Per slot triple, the index of its leaf run (runs end at terminators)."""
    run = np.cumsum(is_term) - is_term                 # per slot: terminators before it
    return run[~is_term][::3]


def check_is_host_tree(flat, info, host, mesh, zero_sign_free=False):
    """The issue's equalities between a device SAH export and vrhip_build_flat's tree.
    zero_sign_free: a box value that is zero may differ in its sign (vrhip.h's one exception)."""
    assert flat["bvh"].shape == host["bvh"].shape
    if zero_sign_free:
        rows = lambda f: f["bvh"].reshape(-1, 4, 4)                      # noqa: E731
        assert rows(flat)[:, 3].tobytes() == rows(host)[:, 3].tobytes()
        assert (rows(flat)[:, :3] + np.float32(0.0)).tobytes() == (rows(host)[:, :3] + np.float32(0.0)).tobytes()
    else:
        assert flat["bvh"].tobytes() == host["bvh"].tobytes()
    depth, n_nodes = validate_flat(flat)
    assert (depth, n_nodes) == validate_flat(host)
    assert info == (depth, n_nodes, len(flat["verts"]))
    for k in ("verts", "normals", "tangents", "uvs"):
        assert flat[k].shape == host[k].shape, k
    d_term, d_rows = slot_rows(flat)
    h_term, h_rows = slot_rows(host)
    assert np.array_equal(d_term, h_term)
    # triangle index of every slot triple (rows are distinct in these meshes)
    index = {row.tobytes(): i for i, row in enumerate(expected_triangles(mesh))}
    d_idx = np.array([index[row.tobytes()] for row in d_rows])
    h_idx = np.array([index[row.tobytes()] for row in h_rows])
    leaf = leaf_of_triple(d_term)
    # the same triangles in every leaf run: the host's, sorted within the run, are the device's
    order = np.lexsort((h_idx, leaf))
    assert np.array_equal(h_idx[order], d_idx)
    same_leaf = leaf[1:] == leaf[:-1]
    assert (d_idx[1:][same_leaf] > d_idx[:-1][same_leaf]).all()           # ascending input index


# ---- 1. the host's tree ---------------------------------------------------------
SIZES = sorted({2, 3, 5, 63, 64, 65, 257, 1000, T - 1, T, T + 1, 4 * T + 3})


@pytest.mark.parametrize("max_leaf", [1, 2, 4])
@pytest.mark.parametrize("n_tris", SIZES)
def test_soup_tree_is_the_hosts(native, n_tris, max_leaf):
    mesh = soup(n_tris)
    flat, info = built_export(mesh, max_leaf)
    check_is_host_tree(flat, info, host_flat(("soup", n_tris), mesh, max_leaf), mesh)


@pytest.mark.parametrize("max_leaf", [2, 4])
@pytest.mark.parametrize("knot", [(40, 20), (100, 50)])
def test_knot_tree_is_the_hosts(native, knot, max_leaf):
    mesh = scenes.torus_knot(*knot)
    flat, info = built_export(mesh, max_leaf)
    check_is_host_tree(flat, info, host_flat(("knot",) + knot, mesh, max_leaf), mesh)


@pytest.mark.parametrize("max_leaf", [1, 2, 4])
def test_single_triangle_sits_under_two_leaves(native, max_leaf):
    mesh = soup(1)
    flat, info = built_export(mesh, max_leaf)
    host = host_flat(("soup", 1), mesh, max_leaf)
    assert flat["bvh"].tobytes() == host["bvh"].tobytes()
    for k in ("verts", "normals", "tangents", "uvs"):
        assert flat[k].tobytes() == host[k].tobytes(), k
    assert info == (1, 1, 8)
    is_term, rows = slot_rows(flat)
    assert is_term.tolist() == [False] * 3 + [True] + [False] * 3 + [True]
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], expected_triangles(mesh)[0])


# ---- 2. hard inputs -----------------------------------------------------------
@pytest.mark.parametrize("kind", HARD_KINDS)
def test_hard_inputs_valid_and_bitexact(native, oracle, kind):
    mesh = hard_mesh(kind)
    sc = scenes.make_scene("C2", 64, 48)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    device_build(r, mesh, 2)
    flat, info = r.export_mesh_flat(), r.bvh_info()
    depth, n_nodes = check_boxes_and_leaves(flat, mesh, 2)
    assert info == (depth, n_nodes, len(flat["verts"]))
    if kind in ("identical", "flat_axis"):             # the host's own reference order cannot matter here
        assert flat["bvh"].tobytes() == build_flat(mesh, max_leaf_tris=2)["bvh"].tobytes()
    times = [4242, 4249]
    r.render(frames=2, times=times)
    ga, gr, gd = r.read_accum(), r.read_rgba8(), r.read_depth8()
    r.cleanUp()
    sc = dict(sc, mesh_flat=flat)
    oa, orgba, od, _ = po.render(sc, frames=2, times=times, libm=po.LIBM_PORTABLE)
    assert np.array_equal(ga.view(np.uint32), oa.view(np.uint32))
    assert np.array_equal(gr, orgba) and np.array_equal(gd, od)


# ---- 3. render parity -----------------------------------------------------------
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_render_parity_on_sah_built_knot(native, oracle, name):
    mesh = scenes.torus_knot(100, 50)
    sc = scenes.make_scene(name, 160, 96)
    times = [12345 + 7 * i for i in range(3)]
    r = loaded(sc, mesh)
    flat = r.export_mesh_flat()
    assert r.bvh_info()[0] == validate_flat(flat)[0]
    r.render(frames=3, times=times)
    ga, gr, gd = r.read_accum(), r.read_rgba8(), r.read_depth8()
    osc = dict(sc, mesh_flat=flat)
    oa, orgba, od, _ = po.render(osc, frames=3, times=times, libm=po.LIBM_PORTABLE)
    bitexact(ga, oa, f"{name} accum")
    bitexact(gr, orgba, f"{name} rgba8")
    bitexact(gd, od, f"{name} depth8")
    assert np.any(oa[..., :3] != 0)
    r.set_strict_traversal(True)                       # every pierced box visited: the same image
    r.clearBuffer()
    r.render(frames=3, times=times)
    bitexact(r.read_accum(), ga, f"{name} strict traversal")
    r.cleanUp()
    if name != "C2":
        return
    t4 = times + [99991]                               # a render-service session: two unsynchronised 2-frame calls
    r = loaded(sc, mesh)
    r.set_service(1)
    r.render(frames=2, times=t4[:2], sync=False)
    r.render(frames=2, times=t4[2:], sync=False)
    r.sync()
    sa = r.read_accum()
    assert r.service_info()["served"] >= 1
    r.cleanUp()
    o4, _, _, _ = po.render(osc, frames=4, times=t4, libm=po.LIBM_PORTABLE)
    bitexact(sa, o4, "C2 service session")
    r = VRendererHIP(0)                                # tree independence across builders: the host-built tree
    scenes.load_into(r, sc)
    r.initMesh(build_flat(mesh))
    r.clearBuffer()
    r.render(frames=3, times=times)
    bitexact(r.read_accum(), ga, "C2 host-built tree")
    r.cleanUp()


# ---- 4. determinism -------------------------------------------------------------
def test_two_sah_builds_are_byte_identical(native):
    mesh = scenes.torus_knot(60, 30)
    a, ia = built_export(mesh)
    b, ib = built_export(mesh)
    assert ia == ib
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- 5. mid size ----------------------------------------------------------------
def test_mid_size_knot(native):
    mesh = scenes.torus_knot(300, 150)                 # 90k triangles: both regimes, many levels deep
    flat, info = built_export(mesh)
    host = build_flat(mesh, max_leaf_tris=2)
    assert flat["bvh"].tobytes() == host["bvh"].tobytes()
    depth, n_nodes = validate_flat(host)
    assert info[:2] == (depth, n_nodes) and validate_flat(flat) == (depth, n_nodes)


# ---- 6. errors and switching ------------------------------------------------------
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
    for bad, leaf, builder in ((bad_index, 2, "sah"), (nan_vertex, 2, "sah"), (empty, 2, "sah"), (mesh, 128, "sah"),
                               (mesh, 2, 7)):
        with pytest.raises(VRHIPError) as e:
            device_build(r, bad, leaf, builder)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        device_build(r, mesh, 2, "lbvh")
    assert r.bvh_info() == info
    r.clearBuffer()
    r.render(frames=2, times=[1, 2])
    assert np.array_equal(r.read_accum().view(np.uint32), first.view(np.uint32))
    r.cleanUp()


def test_multi_device_context_is_refused(native):
    import torch
    mesh = scenes.torus_knot(8, 6)
    r = VRendererHIP([0])
    r.init(64, 48)
    with pytest.raises(VRHIPError) as e:
        r.initMeshDevice(torch.from_numpy(mesh["positions"]).cuda(0),
                         torch.from_numpy(np.ascontiguousarray(mesh["tris"], np.int32)).cuda(0), builder="sah")
    assert e.value.code == -1 and "multi-device" in str(e.value)
    r.cleanUp()


def test_switching_builders_between_unsynchronised_renders(native):
    a, b = scenes.torus_knot(40, 20), scenes.torus_knot(30, 12)
    sc = scenes.make_scene("C2", 64, 48)
    steps = [(a, "morton", [1, 2]), (b, "sah", [3, 4]), (a, "morton", [5, 6])]
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.set_service(1)
    got = []
    for mesh, builder, times in steps:
        device_build(r, mesh, 2, builder)              # the previous step's last render is still unsynchronised
        r.clearBuffer()
        r.render(frames=2, times=times, sync=False)
        r.sync()
        got.append((r.export_mesh_flat(), r.bvh_info(), r.read_accum()))
        r.render(frames=2, times=[t + 100 for t in times], sync=False)
    r.sync()
    assert r.service_info()["refused"] == 0
    r.cleanUp()
    for (mesh, builder, times), (flat, info, accum) in zip(steps, got):
        r = loaded(sc, mesh, builder)
        r.set_service(1)
        r.render(frames=2, times=times)
        assert r.bvh_info() == info
        want = r.export_mesh_flat()
        for k in flat:
            assert flat[k].tobytes() == want[k].tobytes(), (builder, k)
        assert np.array_equal(accum.view(np.uint32), r.read_accum().view(np.uint32)), builder
        r.cleanUp()


# ---- 7. the default is unchanged --------------------------------------------------
def test_default_builder_is_morton(native):
    mesh = scenes.torus_knot(40, 20)
    a, ia = built_export(mesh, 2, builder=None)        # initMeshDevice without the argument
    b, ib = built_export(mesh, 2, builder="morton")
    s, _ = built_export(mesh, 2, builder="sah")
    assert ia == ib
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["bvh"].tobytes() != s["bvh"].tobytes()
