"""The device builders, the refit, the renders and the ray queries at the
extremes of float (tests/extreme_cases.py): what vrhip.h promises for every
finite input -- valid trees with exact boxes, the host's tree byte for byte
from the SAH builder, exact boxes and the host's cost after a refit, renders
equal to the portable oracle on the export, and ray records that are the host
walk's in both traversal modes -- on meshes whose extents, centroids and
products overflow or are denormal, and on rays of every magnitude a float
holds.  The host walk and the meshes are pinned without a device in
test_extreme_cpu.py."""
import functools

import numpy as np
import pytest

import extreme_cases as ec
import pyoracle as po
from device_mesh_cases import BUILDERS, device_build, fresh, hard_mesh, soup
from extreme_cases import EXTREME_KINDS, assert_same_records, check_boxes_and_leaves, extreme_mesh, extreme_ray_set
from ray_query_cases import NO_HIT, same_bits, u32
from test_gpu_device_sah import check_is_host_tree
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, build_flat, flat_sah_cost, flat_trace_rays, scenes

pytestmark = pytest.mark.gpu

N_RAYS = 2048
UPLOADS = BUILDERS + ["host"]
BUILD_KINDS = EXTREME_KINDS + ["far"]


def mesh_of(kind):
    if kind == "soup200":
        return soup(200)
    if kind.startswith("offset"):
        return ec.offset_mesh(float(kind[6:]))
    return hard_mesh(kind) if kind == "far" else extreme_mesh(kind)


def dev(a, dtype=np.float32):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda(0)


@pytest.fixture(scope="module")
def r(native):
    r = fresh()
    yield r
    r.cleanUp()


def index_words(flat):
    return flat["bvh"].reshape(-1, 4, 4)[:, 3].copy().view(np.uint32)


# ---- 1. the builders ----------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [1, 3])
@pytest.mark.parametrize("kind", BUILD_KINDS)
@pytest.mark.parametrize("builder", BUILDERS)
def test_builders_at_the_extremes(r, builder, kind, leaf):
    mesh = mesh_of(kind)
    device_build(r, mesh, leaf, builder)
    flat, info = r.export_mesh_flat(), r.bvh_info()
    depth, n_nodes = check_boxes_and_leaves(flat, mesh, leaf)   # valid, every triangle once, exact boxes
    assert info == (depth, n_nodes, len(flat["verts"]))
    if builder == "sah":                               # the host's tree, its leaves' triangles in ascending input index
        check_is_host_tree(flat, info, build_flat(mesh, max_leaf_tris=leaf), mesh, zero_sign_free=True)
    device_build(r, mesh, leaf, builder)
    again = r.export_mesh_flat()
    assert r.bvh_info() == info
    for k in flat:
        assert flat[k].tobytes() == again[k].tobytes(), k


def test_a_tree_the_host_upload_refuses_is_refused_by_the_sah_builder(native):
    """depth_cap_mesh's SAH tree ends in a leaf of 130 triangles at the depth
    cap.  vrhip_build_flat builds it, the upload of that tree answers
    VRHIP_ERR_BVH, and so does the device's SAH build of the same mesh; the
    mesh resident before still renders as it did."""
    mesh = ec.depth_cap_mesh()
    flat = build_flat(mesh, max_leaf_tris=2)
    term = np.flatnonzero(u32(flat["verts"][:, 0]) == 0x80000000)
    assert (np.diff(np.concatenate([[-1], term])) - 1).max() == 3 * 130
    q = VRendererHIP(0)
    scenes.load_into(q, scenes.make_scene("C2", 64, 48))
    device_build(q, soup(65), 2, "sah")
    q.render(frames=1, times=[5])
    before, info = q.read_accum(), q.bvh_info()
    for refused in (lambda: q.initMesh(flat), lambda: device_build(q, mesh, 2, "sah")):
        with pytest.raises(VRHIPError) as e:
            refused()
        assert e.value.code == -4 and q.bvh_info() == info
        q.clearBuffer()
        q.render(frames=1, times=[5])
        assert q.read_accum().tobytes() == before.tobytes()
    q.cleanUp()


# ---- 2. the refit ---------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
def test_refit_through_the_extremes_and_back(r, builder):
    """The ordinary 200-soup's tree, refit to the positions of big, huge and
    tiny and back: the topology never changes, every box is exact after every
    step, the device's cost is the host's on the export, and the way back ends
    where it began."""
    leaf = 2
    mesh = soup(200)
    device_build(r, mesh, leaf, builder)
    first, info = r.export_mesh_flat(), r.bvh_info()
    steps = [(k, extreme_mesh(k)["positions"]) for k in ("big", "huge", "tiny")] + [("back", mesh["positions"])]
    for name, P in steps:
        r.refitMeshDevice(dev(P))
        after = r.export_mesh_flat()
        assert r.bvh_info() == info
        assert index_words(after).tobytes() == index_words(first).tobytes(), name
        check_boxes_and_leaves(after, dict(mesh, positions=P), leaf)
        got, want = r.bvh_sah_cost(), flat_sah_cost(after)
        print(builder, name, "device cost", repr(got), "host", repr(want))
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (name, got, want)
    for k in first:
        assert after[k].tobytes() == first[k].tobytes(), k


# ---- 3. renders -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", EXTREME_KINDS)
@pytest.mark.parametrize("builder", BUILDERS)
def test_renders_on_extreme_trees_are_bitexact(native, oracle, builder, kind):
    """Ordinary camera rays through a tree whose fp16 boxes are infinite (big,
    huge, wide) or whose edges are denormal (tiny): both walks against the
    portable oracle on the exported tree."""
    mesh = extreme_mesh(kind)
    times = [4242, 4249]
    for name in ("C2", "C3"):
        sc = scenes.make_scene(name, 64, 48)
        q = VRendererHIP(0)
        scenes.load_into(q, sc)
        device_build(q, mesh, 2, builder)
        flat = q.export_mesh_flat()
        oa, orgba, od, _ = po.render(dict(sc, mesh_flat=flat), frames=2, times=times, libm=po.LIBM_PORTABLE)
        for strict in (False, True):
            q.set_strict_traversal(strict)
            q.clearBuffer()
            q.render(frames=2, times=times)
            what = f"{name} {kind} {builder} strict={strict}"
            assert np.array_equal(q.read_accum().view(np.uint32), oa.view(np.uint32)), what
            assert np.array_equal(q.read_rgba8(), orgba) and np.array_equal(q.read_depth8(), od), what
        q.cleanUp()


# ---- 4. ray queries ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def query_case(name):
    """(mesh, rays): computed once, shared by the uploads, never written."""
    if name.startswith("nan-"):
        return ec.nan_plane_case(both=name == "nan-both")
    if name.startswith("near-"):
        mesh = mesh_of(name[5:])
        return mesh, ec.near_ray_set(np.ascontiguousarray(mesh["positions"][mesh["tris"].astype(np.int64)]), 600)
    mesh = mesh_of(name)
    V = np.ascontiguousarray(mesh["positions"][mesh["tris"].astype(np.int64)])
    return mesh, extreme_ray_set(V, N_RAYS)


def trace(r, rays, any_hit=False, tmax=True):
    out = r.traceRays(dev(rays["origins"]), dev(rays["dirs"]), dev(rays["tmax"]) if tmax else None, any_hit=any_hit)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_three_agree(r, mesh, rays, uploaded_flat, what):
    """Device culled, device strict and the host walk on the export: closest
    and any-hit, with and without tmax.  prim is compared through the data for
    a device build (the caller's triangle) and directly for a host upload."""
    flat = r.export_mesh_flat()
    tris = None if uploaded_flat is not None else np.ascontiguousarray(mesh["positions"][mesh["tris"].astype(np.int64)])
    hits = 0
    for tmax in (True, False):
        t0 = rays["tmax"] if tmax else np.full(len(rays["tmax"]), NO_HIT, np.float32)
        want = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"] if tmax else None)
        hit = want["prim"] >= 0
        hits += int(hit.sum())
        got = {}
        for strict in (False, True):
            r.set_strict_traversal(strict)
            got[strict] = trace(r, rays, tmax=tmax)
            anyh = trace(r, rays, any_hit=True, tmax=tmax)
            w = f"{what} tmax={tmax} strict={strict}"
            assert_same_records(got[strict], want, w, prim=uploaded_flat is not None)
            assert same_bits(got[strict]["t"][~hit], t0[~hit]) and (got[strict]["prim"][~hit] == -1).all(), w
            assert ((anyh["prim"] >= 0) == hit).all(), w + " any-hit"
            assert not anyh["prim"][hit].any() and not any(u32(anyh[k][hit]).any() for k in ("t", "u", "v")), w
            assert same_bits(anyh["t"][~hit], t0[~hit]) and (anyh["prim"][~hit] == -1).all(), w
            assert not u32(anyh["u"][~hit]).any() and not u32(anyh["v"][~hit]).any(), w
            if tris is not None:                       # the triangle the device names holds the slot's vertices
                p = got[strict]["prim"][hit]
                assert ((p >= 0) & (p < len(tris))).all(), w
                slot = want["prim"][hit]
                held = np.stack([flat["verts"][slot + k, :3] for k in range(3)], 1)
                assert held.tobytes() == tris[p].tobytes(), w
        r.set_strict_traversal(False)
        assert_same_records(got[False], got[True], f"{what} tmax={tmax}: culled against strict")
    return hits


def upload(r, mesh, how):
    if how == "host":
        flat = build_flat(mesh, 2)
        r.initMesh(flat)
        return flat
    device_build(r, mesh, 2, how)
    return None


@pytest.mark.parametrize("how", UPLOADS)
@pytest.mark.parametrize("name", ["soup200", "big", "far"])
def test_extreme_rays_agree_on_device_and_host(r, name, how):
    mesh, rays = query_case(name)
    hits = check_three_agree(r, mesh, rays, upload(r, mesh, how), f"{name} {how}")
    if name == "soup200":
        assert hits >= 150                             # test_extreme_cpu.py asserts 100 with tmax on the host tree


@pytest.mark.parametrize("how", UPLOADS)
@pytest.mark.parametrize("name", ["soup200", "far", "offset1e3", "offset1e6"])
def test_rays_across_the_culled_walks_reach_agree(r, name, how):
    """extreme_cases.near_ray_set: origins both sides of the distance (8
    extents) at which the query kernel sends a ray through the strict walk, and
    origins a few times the mesh's largest coordinate out, on a centred mesh,
    on one beyond the largest half (every ray strict) and on small meshes 80
    and 80,000 extents from zero, where the coordinates and not the distance
    are what is large."""
    mesh, rays = query_case("near-" + name)
    hits = check_three_agree(r, mesh, rays, upload(r, mesh, how), f"near {name} {how}")
    assert hits >= len(rays["tmax"]) // 2              # of 2 x 600; the walk loses some of the far ones, as the reference does


@pytest.mark.parametrize("how", UPLOADS)
@pytest.mark.parametrize("name", ["nan-both", "nan-one"])
def test_nan_slab_rays_agree_on_device_and_host(r, name, how):
    """Slab arithmetic that is inf - inf.  On both planes of an axis it hides
    every box.  On one plane (nan-one: boxes that straddle 0) the integer span
    reads the NaN's sign: the device sets it and misses every one of these
    rays, although the brute force hits them all; with the sign clear the
    walk would hit them all.  The host walk canonicalises the NaN to the
    device's (vr_raycast.cpp slab_dev), and this test is what says which."""
    mesh, rays = query_case(name)
    hits = check_three_agree(r, mesh, rays, upload(r, mesh, how), f"{name} {how}")
    assert hits == 0
    import torch
    inf = torch.full((1,), float("inf"), device="cuda:0")
    assert (inf - inf).view(torch.int32).item() == -0x400000          # 0xffc00000
