"""Refit of a device-built mesh (vrhip_refit_mesh_device) and the tree's SAH
cost (vrhip_bvh_sah_cost): the topology stays, every box is exact again, the
renders are bit-exact against the portable oracle walking the refit tree, the
cost equals the host's, and a refused refit leaves the mesh as it was."""
import hashlib

import numpy as np
import pytest

import pyoracle as po
from device_mesh_cases import BUILDERS, bitexact, deform, device_build, fresh, loaded, soup
from extreme_cases import check_boxes_and_leaves
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, flat_sah_cost, scenes, validate_flat

pytestmark = pytest.mark.gpu

TERM = 0x80000000


def twist_dirs(D, P, k=0.03):
    """Directions at the points P turned by the same angle (the new normals)."""
    D, a = np.asarray(D, np.float64), k * np.asarray(P, np.float64)[:, 1]
    c, s = np.cos(a), np.sin(a)
    return np.stack([c * D[:, 0] + s * D[:, 2], D[:, 1], -s * D[:, 0] + c * D[:, 2]], -1).astype(np.float32)


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda(0)


def refit(r, positions, normals=None, tangents=None):
    r.refitMeshDevice(dev(positions), dev(normals), dev(tangents))


def index_words(flat):
    return flat["bvh"].reshape(-1, 4, 4)[:, 3].copy().view(np.uint32)


def terminators(flat):
    return np.flatnonzero(flat["verts"][:, 0].copy().view(np.uint32) == TERM)


def root_box(flat):
    n = flat["bvh"].reshape(-1, 4, 4)[0]
    lo = np.minimum([n[0, 0], n[0, 2], n[2, 0]], [n[1, 0], n[1, 2], n[2, 2]])
    hi = np.maximum([n[0, 1], n[0, 3], n[2, 1]], [n[1, 1], n[1, 3], n[2, 3]])
    return lo, hi


def digest(r, times=(1, 2)):
    r.clearBuffer()
    r.render(frames=len(times), times=list(times))
    return hashlib.sha256(r.read_accum().tobytes()).hexdigest()


# ---- 1. exact boxes, unchanged topology ------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("max_leaf", [1, 3])
@pytest.mark.parametrize("n_tris", [1, 2, 5, 65, 257])
def test_refit_keeps_topology_and_makes_exact_boxes(native, n_tris, max_leaf, builder):
    mesh = soup(n_tris, seed=5)
    P = mesh["positions"]
    assert len(np.unique(P, axis=0)) == len(P)         # distinct positions: a slot names one vertex
    r = fresh()
    device_build(r, mesh, max_leaf, builder)
    before, info = r.export_mesh_flat(), r.bvh_info()
    P2 = deform(P)
    refit(r, P2)
    after = r.export_mesh_flat()
    assert r.bvh_info() == info
    assert index_words(before).tobytes() == index_words(after).tobytes()
    term = terminators(before)
    assert np.array_equal(term, terminators(after))
    keep = np.ones(len(before["verts"]), bool)
    keep[term] = False
    # each slot holds the new position of the vertex it held before
    where = {P[v].tobytes(): v for v in range(len(P))}
    slot_vert = np.array([where[p.tobytes()] for p in before["verts"][keep, :3]])
    assert after["verts"][keep, :3].tobytes() == P2[slot_vert].tobytes()
    assert (after["verts"][keep, 3] == 0).all()
    assert after["verts"][term].tobytes() == before["verts"][term].tobytes()
    for k in ("normals", "tangents", "uvs"):           # None keeps what is resident
        assert after[k].tobytes() == before[k].tobytes(), k
    moved = dict(mesh, positions=P2)
    check_boxes_and_leaves(after, moved, max_leaf)     # every child box the min/max of the vertices beneath it
    validate_flat(after)
    # normals and tangents are replaced when given
    rng = np.random.default_rng(11)
    N2 = rng.normal(0, 1, P.shape).astype(np.float32)
    T2 = rng.normal(0, 1, P.shape).astype(np.float32)
    refit(r, P2, N2, T2)
    again = r.export_mesh_flat()
    assert again["normals"][keep, :3].tobytes() == N2[slot_vert].tobytes()
    assert again["tangents"][keep, :3].tobytes() == T2[slot_vert].tobytes()
    assert (again["normals"][keep, 3] == 0).all() and (again["tangents"][keep, 3] == 0).all()
    for k in ("bvh", "verts", "uvs"):
        assert again[k].tobytes() == after[k].tobytes(), k
    for k in ("normals", "tangents"):
        assert again[k][term].tobytes() == before[k][term].tobytes(), k
    refit(r, P2, None, T2[::-1].copy())                # one of the two alone
    third = r.export_mesh_flat()
    assert third["normals"].tobytes() == again["normals"].tobytes()
    assert third["tangents"][keep, :3].tobytes() == T2[::-1][slot_vert].tobytes()
    r.cleanUp()


# ---- 2. identity -------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
def test_refit_to_the_same_positions_changes_nothing(native, builder):
    mesh = scenes.torus_knot(60, 30)
    r = fresh()
    device_build(r, mesh, 2, builder)
    before, cost = r.export_mesh_flat(), r.bvh_sah_cost()
    refit(r, mesh["positions"])
    after = r.export_mesh_flat()
    for k in ("verts", "normals", "tangents", "uvs"):
        assert after[k].tobytes() == before[k].tobytes(), k
    # a box holding both -0 and +0 at an extreme may differ in that zero's sign
    assert (after["bvh"] + np.float32(0.0)).tobytes() == (before["bvh"] + np.float32(0.0)).tobytes()
    assert np.float64(r.bvh_sah_cost()).tobytes() == np.float64(cost).tobytes()
    r.cleanUp()


# ---- 3. render parity ---------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_render_parity_after_refit(native, oracle, name, builder):
    mesh = scenes.torus_knot(100, 50)
    sc = scenes.make_scene(name, 160, 96)
    times = [12345 + 7 * i for i in range(3)]
    r = loaded(sc, mesh, builder)
    lo0, hi0 = root_box(r.export_mesh_flat())
    r.render(frames=3, times=times)
    img0 = r.read_accum()
    refit(r, deform(mesh["positions"]), twist_dirs(mesh["normals"], mesh["positions"]))
    r.clearBuffer()
    r.render(frames=3, times=times)
    ga, gr, gd = r.read_accum(), r.read_rgba8(), r.read_depth8()
    flat = r.export_mesh_flat()
    oa, orgba, od, _ = po.render(dict(sc, mesh_flat=flat), frames=3, times=times, libm=po.LIBM_PORTABLE)
    bitexact(ga, oa, f"{name} accum")
    bitexact(gr, orgba, f"{name} rgba8")
    bitexact(gd, od, f"{name} depth8")
    # not vacuous: another image, and a root box the old one does not contain
    assert np.any(ga.view(np.uint32) != img0.view(np.uint32))
    lo1, hi1 = root_box(flat)
    assert (lo1 < lo0).any() or (hi1 > hi0).any()
    # every pierced box visited, as the reference walks: stale fp16 boxes or edges would show
    r.set_strict_traversal(True)
    r.clearBuffer()
    r.render(frames=3, times=times)
    bitexact(r.read_accum(), oa, f"{name} strict traversal accum")
    bitexact(r.read_rgba8(), orgba, f"{name} strict traversal rgba8")
    bitexact(r.read_depth8(), od, f"{name} strict traversal depth8")
    r.cleanUp()


# ---- 4. the refit tree loses no triangle ---------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
def test_refit_tree_equals_brute_force(native, oracle, builder):
    mesh = soup(300, seed=5)
    mesh.update(normals=np.tile([0, 0, 1], (900, 1)).astype(np.float32),
                tangents=np.tile([1, 0, 0], (900, 1)).astype(np.float32))
    r = fresh()
    device_build(r, mesh, 3, builder)
    refit(r, deform(mesh["positions"]))
    flat = r.export_mesh_flat()
    r.cleanUp()
    sc = scenes.make_scene("C2", 48, 32)
    sc["mesh_flat"] = flat
    a, _, _, _ = po.render(sc, frames=1)
    b, _, _, _ = po.render(sc, frames=1, brute_force=True)
    assert np.any(a[..., :3] != 0)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 5. between unsynchronised renders -------------------------------------------------
def test_refit_between_unsynchronised_renders(native, oracle):
    mesh = scenes.torus_knot(40, 20)
    sc = scenes.make_scene("C2", 64, 48)
    t4 = [3, 4, 5, 99991]
    r = loaded(sc, mesh, "sah")
    r.set_service(1)
    r.render(frames=2, times=[1, 2], sync=False)
    s0 = r.service_info()["sessions"]
    refit(r, deform(mesh["positions"]))
    r.clearBuffer()
    r.render(frames=2, times=t4[:2], sync=False)
    r.render(frames=2, times=t4[2:], sync=False)
    r.sync()
    got = r.read_accum()
    si = r.service_info()
    assert si["sessions"] > s0 >= 1 and si["refused"] == 0     # the refit closed the first session
    flat = r.export_mesh_flat()
    r.cleanUp()
    o4, _, _, _ = po.render(dict(sc, mesh_flat=flat), frames=4, times=t4, libm=po.LIBM_PORTABLE)
    bitexact(got, o4, "C2 service session after a refit")


# ---- 6. cost ---------------------------------------------------------------------------
# The device sums fewer than 10^4 positive fp64 terms in another order than the
# host: below 10^4 * 2^-53 ~ 1e-12 relative (tests/test_refit_cpu.py).
REL = 1e-9


def test_sah_cost_equals_the_hosts_and_grows_under_a_refit(native):
    mesh = scenes.torus_knot(60, 30)
    P2 = deform(mesh["positions"])
    costs = {}
    for builder in BUILDERS:
        r = fresh()
        device_build(r, mesh, 2, builder)
        for stage in ("built", "refit"):
            if stage == "refit":
                refit(r, P2)
            got, again, want = r.bvh_sah_cost(), r.bvh_sah_cost(), flat_sah_cost(r.export_mesh_flat())
            print(builder, stage, "device", got, "host", want)
            assert np.float64(got).tobytes() == np.float64(again).tobytes()
            assert np.isfinite(want) and abs(got - want) <= REL * want
            costs[builder, stage] = got
        r.cleanUp()
    r = fresh()
    device_build(r, dict(mesh, positions=P2), 2, "sah")
    rebuilt = r.bvh_sah_cost()
    r.cleanUp()
    print("sah rebuilt on the deformed knot", rebuilt)
    assert costs["sah", "refit"] > rebuilt


def test_sah_cost_of_a_host_uploaded_tree(native):
    flat = scenes.knot_flat(40, 20)
    r = fresh()
    r.initMesh(flat)
    got, want = r.bvh_sah_cost(), flat_sah_cost(flat)
    r.cleanUp()
    assert abs(got - want) <= REL * want


# ---- 7. refusals leave the mesh as it was ------------------------------------------------
def test_refusals_leave_the_resident_mesh(native):
    mesh = scenes.torus_knot(40, 20)
    P = mesh["positions"]
    sc = scenes.make_scene("C2", 64, 48)
    r = loaded(sc, mesh, "sah")
    before, first = r.export_mesh_flat(), digest(r)

    def unchanged():
        after = r.export_mesh_flat()
        for k in before:
            assert after[k].tobytes() == before[k].tobytes(), k
        assert digest(r) == first

    nan = deform(P)
    nan[int(mesh["tris"][5, 2]), 1] = np.nan
    inf = deform(P)
    inf[int(mesh["tris"][-1, 0]), 2] = np.inf
    for bad in (nan, inf, deform(P)[:-1], np.concatenate([P, P[:1]])):      # not finite; the wrong n_verts
        with pytest.raises(VRHIPError) as e:
            refit(r, bad)
        assert e.value.code == -1
        unchanged()
    good = dev(deform(P))
    wrong = [dict(positions=good.cpu()), dict(positions=good.double()), dict(positions=good.t().contiguous().t()),
             dict(positions=good[:, :2].contiguous()), dict(positions=good, normals=good[:-1]),
             dict(positions=good, tangents=good.double()), dict(positions=np.asarray(P))]
    for kw in wrong:                                     # device, dtype, contiguity, shape, not a tensor
        with pytest.raises(ValueError):
            r.refitMeshDevice(**kw)
        unchanged()
    # a mesh uploaded from the host keeps no index data
    r.initMesh(scenes.knot_flat(40, 20))
    with pytest.raises(VRHIPError) as e:
        refit(r, P)
    assert e.value.code == -1
    r.cleanUp()
    r = fresh()                                          # no mesh
    with pytest.raises(VRHIPError) as e:
        refit(r, P)
    assert e.value.code == -1
    r.cleanUp()
    r = VRendererHIP([0])                                # a multi-device context of one device
    r.init(64, 48)
    with pytest.raises(VRHIPError) as e:
        refit(r, P)
    assert e.value.code == -1 and "multi-device" in str(e.value)
    r.cleanUp()
