"""Every kernel that walks the mesh, with its traversal stack filled to the
last entry.

The kernels are built with 16, 24, 32 and 64 stack entries for trees of depth
up to 15, 23, 30 and 62 (vr_ctx.hpp mesh_stack_entries), and a walk of a tree
of depth D can need D + 1: no slack at 15, 23, 30 and 62.  An entry too many
would not fault, it would land in the LDS behind the stack and show as wrong
hits.  The trees of tests/stack_cases.py fill the stack (test_stack_cpu.py
shows that they do, that the yardsticks used here agree on them, and that a
stack one entry short changes a quarter of every image and ray set); here
every launch kind, the small-launch kernels with their helper lanes, the
counted and the profiled render and the four queries run on them at the last
depth of each size and the first of the next, in both walks.  Every tree is a
host upload within the documented limits; the one deeper than 62 is refused.

Every comparison is of uint32 words or bytes.
"""
import os

import numpy as np
import pytest

import shade_cases as sh
import stack_cases as st
import surface_cases as sf
from ray_query_cases import flat_triangles
from test_gpu_phase_prio import _run, _same
from test_gpu_ray_query import dev, same_records, trace
from test_gpu_surface import same as same_records28
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, flat_trace_rays, scenes

pytestmark = pytest.mark.gpu

FRAMES = 3
N_RAYS = 512
COUNTED_DEPTHS = (30, 31, 62)
WALKS = ((False, "culled"), (True, "strict"))


def _id(case):
    return "-".join(str(x) for x in case)


def _oracle(sc, frames):
    ref = st.oracle_render(sc, frames)[:3]
    assert np.any(ref[0][..., :3] != 0)
    return ref


def _writable(rays):
    return {k: np.array(v) for k, v in rays.items()}       # copies: the shared ray sets are read-only


def _loaded(sc, strict=False):
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.set_strict_traversal(strict)
    return r


def _run_graph(sc, frames, strict):
    """Synchronous one-frame calls with the one-frame graph on (read when the
    context is made) and kernel timing off, as test_gpu_service.py selects it."""
    old = os.environ.get("VRHIP_GRAPH")
    os.environ["VRHIP_GRAPH"] = "1"
    try:
        r = _loaded(sc, strict)
    finally:
        if old is None:
            del os.environ["VRHIP_GRAPH"]
        else:
            os.environ["VRHIP_GRAPH"] = old
    try:
        r.set_service(0)
        r.set_kernel_timing(False)
        kinds = []
        for k in range(frames):
            r.render(frames=1, times=[sc["time"] + k], sync=True)
            kinds.append(r.last_launch_info()["kind"])
        assert r.getFrameCount() == frames
        return (r.read_accum(), r.read_rgba8(), r.read_depth8()), kinds
    finally:
        r.cleanUp()


# ---- renders against the portable oracle --------------------------------------------------------
@pytest.mark.parametrize("case", st.render_cases(), ids=_id)
def test_renders_equal_the_oracle(native, oracle, case):
    """Accumulation, RGBA8 and depth8 of every launch kind, in both walks.  A
    tree deeper than 30 takes the 64-entry generic kernels, which the render
    service does not hold: a session is then plain launches."""
    kind, depth, cfg = case
    sc = st.scene(st.tree(kind, depth), cfg)
    ref = _oracle(sc, FRAMES)
    session = "service" if depth <= 30 else "path_pool"
    for strict, walk in WALKS:
        got, kinds = _run(sc, [FRAMES], service=0, strict=strict)
        assert kinds == ["path_pool"]
        _same(got, ref, sc, f"{walk}, {FRAMES} frames in one launch")
        got, kinds = _run(sc, [2, 1], service=1, strict=strict)
        assert kinds == [session, session], kinds
        _same(got, ref, sc, f"{walk}, a session of two calls")
        got, _ = _run(sc, [1] * FRAMES, service=0, sync=True, strict=strict)
        _same(got, ref, sc, f"{walk}, one frame per synchronous call")
        got, kinds = _run_graph(sc, FRAMES, strict)
        assert "path_pool_graph" in kinds, kinds
        _same(got, ref, sc, f"{walk}, one-frame graphs")


def test_the_stack_size_follows_the_depth(native):
    r = _loaded(st.scene(st.comb_tree(15)))
    try:
        for depth in st.DEPTHS:
            r.initMesh(st.comb_tree(depth))
            assert r.bvh_info()[0] == depth
    finally:
        r.cleanUp()


# ---- the small-launch kernels: helper lanes take an owner's top entry ----------------------------
@pytest.mark.parametrize("cfg", ["C2", "C3"])
@pytest.mark.parametrize("depth", [15, 30, 62])
def test_small_one_frame_calls(native, oracle, depth, cfg):
    """One-frame calls on images far smaller than the resident pool, as
    test_tiny_one_frame_calls_bitexact makes them, back to back on one stream
    and on three."""
    for (w, h), overlap in zip(st.SMALL_IMAGES, (1, 0)):
        sc = st.scene(st.comb_tree(depth), cfg, w, h)
        ref = _oracle(sc, FRAMES)
        for strict, walk in WALKS:
            r = _loaded(sc, strict)
            try:
                r.set_overlap(overlap)
                for k in range(FRAMES):
                    r.render(frames=1, times=[sc["time"] + k], sync=False)
                r.sync()
                assert r.getFrameCount() == FRAMES
                got = r.read_accum(), r.read_rgba8(), r.read_depth8()
            finally:
                r.cleanUp()
            _same(got, ref, sc, f"{w}x{h} {walk}")


# ---- the counted and the profiled render ----------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C2", "C3"])
@pytest.mark.parametrize("depth", COUNTED_DEPTHS)
def test_counts_equal_the_oracle_s(native, oracle, depth, cfg):
    """The strict walk visits the oracle's nodes and tests its triangles,
    ray for ray in total: a lost or an invented stack entry shows here even
    where the image survives.  The image of the counting kernel is the oracle's too."""
    sc = st.scene(st.comb_tree(depth), cfg)
    ref = st.oracle_render(sc, 1, count=True)
    want = ref[3]
    assert want["max_stack"] == depth
    r = _loaded(sc, strict=True)
    try:
        g = r.render_counted(frames=1, time_seed=sc["time"])
        got = r.read_accum(), r.read_rgba8(), r.read_depth8()
        r.set_strict_traversal(False)
        r.clearBuffer()
        gc = r.render_counted(frames=1, time_seed=sc["time"])
    finally:
        r.cleanUp()
    for k in ("rays", "node_visits", "tri_tests", "hdr_fetches", "brdf_fetches"):
        assert g[k] == want[k], (k, g[k], want[k])
    assert gc["rays"] == want["rays"] and gc["node_visits"] <= want["node_visits"]
    _same(got, ref[:3], sc, "the counted render")


@pytest.mark.parametrize("cfg", ["C2", "C3"])
@pytest.mark.parametrize("depth", COUNTED_DEPTHS)
def test_the_profiled_render_is_the_production_render(native, oracle, depth, cfg):
    sc = st.scene(st.comb_tree(depth), cfg)
    ref = _oracle(sc, 2)
    times = [sc["time"], sc["time"] + 1]
    for strict, walk in WALKS:
        base, _ = _run(sc, [2], service=0, strict=strict)
        r = _loaded(sc, strict)
        try:
            e = r.render_profiled(frames=2, times=times)
            got = r.read_accum(), r.read_rgba8(), r.read_depth8()
        finally:
            r.cleanUp()
        _same(got, base, sc, f"{walk}: profiled against production")
        _same(got, ref, sc, f"{walk}: profiled against the oracle")
        assert e["mesh_hits"] > 0 and e["tri_loads"] >= e["tri_tests"] > 0


# ---- queries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,depth", [(k, d) for k, d, cfg in st.query_cases() if cfg == "C2"], ids=lambda v: str(v))
def test_ray_queries_equal_the_host_walk(native, kind, depth):
    """traceRays on the spine rays: closest hit and any-hit, with tmax and
    without, culled and strict, against the host walk on the export."""
    flat = st.tree(kind, depth)
    rays = _writable(st.rays_of(kind, depth, N_RAYS))
    r = _loaded(st.scene(flat))
    try:
        assert r.bvh_info()[0] == depth
        got = {}
        for strict, walk in WALKS:
            r.set_strict_traversal(strict)
            for tmax in (True, False):
                got[strict, tmax] = trace(r, rays, tmax=tmax)
                want = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"] if tmax else None)
                same_records(got[strict, tmax], want, f"{walk} tmax={tmax}")
                assert (got[strict, tmax]["prim"] == want["prim"]).all()
                hit = want["prim"] >= 0
                any_got = trace(r, rays, any_hit=True, tmax=tmax)
                any_want = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"] if tmax else None, any_hit=True)
                same_records(any_got, any_want, f"{walk} tmax={tmax} any-hit")
                assert (any_got["prim"] == any_want["prim"]).all() and ((any_got["prim"] >= 0) == hit).all()
            # the export is the resident tree flattened anew (its nodes and leaf runs in that flatten's order):
            # the host walk on it returns the same records, and at its prim the triangle the upload holds at ours
            export = r.export_mesh_flat()
            on_export = flat_trace_rays(export, rays["origins"], rays["dirs"], rays["tmax"])
            same_records(got[strict, True], on_export, f"{walk} against the walk on the export")
            held = lambda f, s: np.stack([f["verts"][s + k, :3] for k in range(3)], 1).tobytes()     # noqa: E731
            h = on_export["prim"] >= 0
            assert held(export, on_export["prim"][h]) == held(flat, got[strict, True]["prim"][h]), walk
        r.set_strict_traversal(False)
        assert len(set(want["prim"][hit].tolist())) >= depth / 2 and 0 < (~hit).sum()
        below = np.array(st.TMAX_KINDS)[np.arange(N_RAYS) % 8] == "below"
        assert (got[False, True]["prim"][below] == -1).all() and (got[False, False]["prim"][below] >= 0).sum() > below.sum() / 2
    finally:
        r.cleanUp()


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_rgbw(got, want, what):
    bad = np.flatnonzero((_u32(got) != _u32(want)).any(-1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} results differ (first {bad[:5].tolist()}: " \
                          f"{got[bad[:2]].tolist()} against {want[bad[:2]].tolist()})"


@pytest.mark.parametrize("case", st.query_cases(), ids=_id)
def test_radiance_surface_and_shade_queries(native, oracle, case):
    """On the spine rays, in both walks: traceRadiance against the oracle's
    trace, traceSurface against the oracle's intersect_scene
    (surface_driver.c), shadeSurface(traceSurface) against traceRadiance, and
    shadeSurface of the yardstick's records against shade_driver.c."""
    import radiance_cases as rc
    import torch
    q = st.query_case(*case)
    ok = q["kept"]
    o, d = dev(np.array(q["origins"])), dev(np.array(q["dirs"]))
    s = torch.from_numpy(np.array(q["seeds"]).view(np.int32)).cuda(0)
    records = torch.from_numpy(np.array(q["records"]).view(np.float32)).cuda(0)
    r = _loaded(q["scene"])
    try:
        for strict, walk in WALKS:
            r.set_strict_traversal(strict)
            hits = r.traceSurface(o, d)
            got = np.ascontiguousarray(hits["record"].cpu().numpy()).view(np.uint32)
            same_records28(got[ok], q["records"][ok], f"{walk} traceSurface")
            for k in (1, 2):
                radiance = r.traceRadiance(o, d, s, samples=k).cpu().numpy()
                _same_rgbw(radiance[ok], rc.record_of(q["paths"], k)[ok], f"{walk} traceRadiance samples {k}")
                shaded = r.shadeSurface(hits["record"], d, s, samples=k).cpu().numpy()
                assert not _u32(shaded[:, 3]).any()
                _same_rgbw(shaded[ok, :3], radiance[ok, :3], f"{walk} shadeSurface(traceSurface) samples {k}")
                given = r.shadeSurface(records, d, s, samples=k).cpu().numpy()
                _same_rgbw(given[ok], sh.result_of(q["shaded"], k)[ok], f"{walk} shadeSurface against the driver samples {k}")
        r.set_strict_traversal(False)
        assert np.any(radiance[ok, :3] != 0) and (q["records"][:, sf.KIND] == sf.MESH).sum() > len(ok) / 2
    finally:
        r.cleanUp()


# ---- ties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", st.TIES)
@pytest.mark.parametrize("depth", st.TIE_DEPTHS)
def test_ties(native, oracle, depth, where):
    """Coincident triangles at the end of root paths of `depth` levels, or of
    1 level against `depth`: both walks return the host walk's triangle, and
    the render, in which the two differ by their normals, is the oracle's."""
    flat = st.tie_comb(depth, where)
    rays = _writable(st.spine_rays(flat, N_RAYS))
    winner, loser = st.tie_slots(depth, where)
    sc = st.scene(flat)
    r = _loaded(sc)
    try:
        want = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"])
        for strict, walk in WALKS:
            r.set_strict_traversal(strict)
            got = trace(r, rays)
            same_records(got, want, f"{where} {walk}")
            assert (got["prim"] == want["prim"]).all(), f"{where} {walk}"
        assert (want["prim"] == winner).sum() >= N_RAYS / 4 and (want["prim"][rays["kind"] == "spine"] != loser).all()
    finally:
        r.cleanUp()
    ref = _oracle(sc, FRAMES)
    for strict, walk in WALKS:
        got, _ = _run(sc, [FRAMES], service=0, strict=strict)
        _same(got, ref, sc, f"{where} {walk}")


# ---- the refusal ------------------------------------------------------------------------------------------
def test_a_tree_deeper_than_62_is_refused(native):
    """The depth-63 comb is a valid tree that no kernel's stack holds: initMesh
    answers VRHIP_ERR_BVH and the mesh resident before renders as it did."""
    sc = st.scene(st.comb_tree(62))
    r = _loaded(sc)
    try:
        r.render(frames=1, times=[5])
        before, info = r.read_accum(), r.bvh_info()
        assert info[0] == 62
        with pytest.raises(VRHIPError) as e:
            r.initMesh(st.comb_tree(63))
        assert e.value.code == -4 and r.bvh_info() == info
        r.clearBuffer()
        r.render(frames=1, times=[5])
        assert r.read_accum().tobytes() == before.tobytes()
        _, V = flat_triangles(r.export_mesh_flat())
        assert len(V) == 63
    finally:
        r.cleanUp()
