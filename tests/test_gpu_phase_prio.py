"""Scheduling of the Cornell-box mesh path kernels (vr_kernel.hpp
VR_PHASE_PRIO: a wave's issue priority follows its phase, traversal above
shading): how a wave is scheduled may not change a bit of any image, and the
same cases guard any later change to when the walk reads its stack.

Bit-exact small frames: C2 (the exact specialisation) and C2D (the Cornell
mesh class kernel) through a service session, launch by launch and one frame
per call, against each other and the portable-libm oracle.  192x160 holds
about four paths per resident lane over the six frames, so lanes retire and
restart inside a wave (test_gpu_retire_order.py).

The pop at its edges: the smallest trees (one triangle, two triangles in one
leaf) and a tree at the deepest level of the 16-entry stack class (depth 15:
sixteen similar triangles shrinking four-fold towards a corner, so every SAH
split peels the largest off), culled and strict walks against the oracle.

Priority left clean: renders of other kernels in the same context right after
a C2 service session.
"""
import numpy as np
import pytest

import pyoracle as po
from vrenderer_pathtracer_amd import VRendererHIP, scenes
from vrenderer_pathtracer_amd.renderer import build_flat, validate_flat

pytestmark = pytest.mark.gpu

CALLS = [3, 3]


def _oracle(oracle, sc, frames):
    ref = oracle.render(sc, frames=frames, times=[sc["time"] + k for k in range(frames)], libm=po.LIBM_PORTABLE)[:3]
    for a in ref:
        a.setflags(write=False)
    return ref


def _render(r, sc, calls, sync):
    """`calls` render calls on a loaded renderer; accum, RGBA8, depth and the launch kinds."""
    t, kinds = sc["time"], []
    for n in calls:
        r.render(frames=n, times=[t + k for k in range(n)], sync=sync)
        kinds.append(r.last_launch_info()["kind"])
        t += n
    r.sync()
    assert r.getFrameCount() == sum(calls)
    return (r.read_accum(), r.read_rgba8(), r.read_depth8()), kinds


def _run(sc, calls, service, sync=False, strict=False):
    r = VRendererHIP(0)
    try:
        scenes.load_into(r, sc)
        r.set_service(service)
        r.set_strict_traversal(strict)
        return _render(r, sc, calls, sync)
    finally:
        r.cleanUp()


def _same(got, ref, sc, what):
    """Equal bit for bit on the rendered area (whole 16x16 tiles)."""
    h, w = sc["height"] // 16 * 16, sc["width"] // 16 * 16
    for g, o, name in zip(got, ref, ("accum", "rgba8", "depth8")):
        g, o = g[:h, :w].reshape(-1, 4), o[:h, :w].reshape(-1, 4)
        if g.dtype == np.float32:
            g, o = g.view(np.uint32), o.view(np.uint32)
        bad = int((g != o).any(-1).sum())
        assert bad == 0, f"{what}, {name}: {bad} of {len(g)} pixels differ"


# ---- bit-exact small frames -------------------------------------------------

@pytest.fixture(scope="module", params=[("C2", 96, 64), ("C2", 192, 160), ("C2D", 96, 64), ("C2D", 192, 160)],
                ids=lambda p: f"{p[0]}-{p[1]}x{p[2]}")
def small_ref(request, oracle):
    cfg, w, h = request.param
    sc = scenes.make_scene(cfg, w, h)
    return sc, _oracle(oracle, sc, sum(CALLS))


def test_small_frames_every_path(native, small_ref):
    """Two calls of three frames in a session, launch by launch, and six
    one-frame calls: all equal the oracle, hence each other."""
    sc, ref = small_ref
    assert np.any(ref[0][..., :3] != 0)
    svc, kinds = _run(sc, CALLS, service=1)
    assert kinds == ["service", "service"]
    _same(svc, ref, sc, "service against the oracle")
    lbl, kinds = _run(sc, CALLS, service=0)
    assert kinds == ["path_pool", "path_pool"]
    _same(lbl, ref, sc, "launch by launch against the oracle")
    one, _ = _run(sc, [1] * sum(CALLS), service=0, sync=True)
    _same(one, ref, sc, "one frame per call against the oracle")
    _same(svc, lbl, sc, "service against launch by launch")
    _same(svc, one, sc, "service against one frame per call")


# ---- the pop at its edges ----------------------------------------------------

def _mesh(tri_pos):
    pos = np.asarray(tri_pos, np.float32).reshape(-1, 3)
    n = len(pos)
    return dict(positions=pos, normals=np.tile(np.float32([[0, 0, 1]]), (n, 1)),
                tangents=np.tile(np.float32([[1, 0, 0]]), (n, 1)), uvs=np.zeros((n, 2), np.float32),
                tris=np.arange(n, dtype=np.uint32).reshape(-1, 3))


def _one_triangle():
    return _mesh([[-12, -8, 0], [12, -8, 0], [0, 12, 4]]), 2


def _two_in_one_leaf():
    return _mesh([[-12, -8, 0], [12, -8, 0], [0, 12, 4], [-10, -6, 3], [10, -6, 3], [0, 10, -3]]), 2


def _deepest_16():
    """Sixteen similar triangles, each a quarter of the last, at one corner:
    areas fall 16-fold per triangle, so every binned-SAH split peels the
    largest off and the tree is a chain, one inner node per level."""
    c, tris = np.float64([-12, -12, -12]), []
    for i in range(16):
        s = 24.0 / 4.0 ** i
        tris += [c + [s, 0.5 * s, 0.0], c + [0.5 * s, s, 0.25 * s], c + [0.5 * s, 0.5 * s, s]]
    return _mesh(tris), 1


EDGE_MESHES = {"one-triangle": (_one_triangle, 1, 1), "two-in-one-leaf": (_two_in_one_leaf, 1, 1),
               "depth-15": (_deepest_16, 15, 15)}


@pytest.fixture(scope="module", params=sorted(EDGE_MESHES), ids=str)
def edge_ref(request, native, oracle):
    make, depth, inner = EDGE_MESHES[request.param]
    mesh, max_leaf = make()
    flat = build_flat(mesh, max_leaf_tris=max_leaf)
    assert validate_flat(flat) == (depth, inner), "the host builder's tree: (depth, inner nodes)"
    sc = scenes.make_scene("C2", 64, 48)
    sc["mesh_flat"] = flat
    return sc, _oracle(oracle, sc, 3)


@pytest.mark.parametrize("service", [1, 0])
def test_pop_at_tree_edges(native, edge_ref, service):
    """Trees of one leaf and a chain at the 16-entry stack's deepest level,
    in the Cornell box: the culled and the strict walk equal the oracle."""
    sc, ref = edge_ref
    culled, kinds = _run(sc, [3], service=service)
    assert kinds == ["service" if service else "path_pool"]
    _same(culled, ref, sc, "culled walk against the oracle")
    strict, _ = _run(sc, [3], service=service, strict=True)
    _same(strict, ref, sc, "strict walk against the oracle")
    _same(culled, strict, sc, "culled against strict")


# ---- priority is left clean ---------------------------------------------------

@pytest.fixture(scope="module")
def after_refs(oracle):
    c2 = scenes.make_scene("C2", 96, 64)
    c1 = scenes.make_scene("C1", 96, 64)
    c3 = scenes.make_scene("C3", 96, 64)
    return (c2, _oracle(oracle, c2, 3)), (c1, _oracle(oracle, c1, 2)), (c3, _oracle(oracle, c3, 2))


def test_other_kernels_after_a_session(native, after_refs):
    """A sphere-only render and a C3 render in the context that just ran a C2
    service session: whatever priority the session's waves ended at, the
    next kernels' images are the oracle's."""
    (c2, ref2), (c1, ref1), (c3, ref3) = after_refs
    r = VRendererHIP(0)
    try:
        scenes.load_into(r, c2)
        r.set_service(1)
        got, kinds = _render(r, c2, [3], sync=False)
        assert kinds == ["service"]
        _same(got, ref2, c2, "C2 session")
        # the same context: the scene changes in place (the knot stays loaded;
        # the example sphere hides it, as in the reference)
        r.useExampleSphere(True)
        r.clearBuffer()
        got, _ = _render(r, c1, [2], sync=True)
        _same(got, ref1, c1, "C1 after the C2 session")
        r.useExampleSphere(False)
        r.useCornellBox(False)
        r.loadHDR(c3["hdr"])
        for key, t in (("tex_diffuse", 0), ("tex_normal", 1), ("tex_specular", 2)):
            r.loadTexture(c3[key], 1.0, t)
        r.clearBuffer()
        got, _ = _render(r, c3, [2], sync=True)
        _same(got, ref3, c3, "C3 after the C2 session")
    finally:
        r.cleanUp()
