"""Radiance along the caller's rays (vrhip_trace_radiance, vr_radiance*.hip).

Two yardsticks.  The oracle's own trace through a camera with up = right = 0
(tests/radiance_cases.py; tied to the reference-pinned renders in
test_radiance_cpu.py): the records equal it bit for bit, compared as uint32,
in both traversal modes, on camera rays (set A) and on rays from random points
in random directions of random length (set B).  And the renderer itself,
independent of the oracle: a scene's camera directions with the seeds render
gives its pixels return the first frame's accumulation and depth image."""
import ctypes
import functools

import numpy as np
import pytest

import flag_lattice as fl
import radiance_cases as rc
from device_mesh_cases import deform, device_build, fresh
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, scenes

pytestmark = pytest.mark.gpu

_live = {}


def dev(a, dtype=np.float32):
    import torch
    a = np.array(a, dtype=dtype, order="C")              # a copy: the shared ray sets are read-only
    if dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda(0)


def renderer(name, mesh="shallow"):
    """One renderer per scene for the whole module; the tests leave its scene
    flags as they found them."""
    key = (name, mesh)
    if key not in _live:
        r = VRendererHIP(0)
        scenes.load_into(r, fl.scene_of(rc.combo_of(name), mesh))
        _live[key] = r
    return _live[key]


@pytest.fixture(scope="module", autouse=True)
def _renderers(native):
    yield
    for r in _live.values():
        r.cleanUp()
    _live.clear()


def trace(r, o, d, s, samples=2):
    out = r.traceRadiance(dev(o), dev(d), dev(s, np.uint32), samples=samples)
    assert out.is_cuda and tuple(out.shape) == (len(o), 4) and str(out.dtype) == "torch.float32"
    return out.cpu().numpy()


def same(got, want, what):
    bad = np.flatnonzero((rc.u32(got) != rc.u32(want)).any(-1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ (first {bad[:5].tolist()}: " \
                          f"{got[bad[:2]].tolist()} against {want[bad[:2]].tolist()})"


def check_against_oracle(r, name, mesh, what):
    for which in ("A", "B"):
        o, d, s = rc.ray_set(which)
        paths, ok = rc.reference(name, which, mesh)
        for k in rc.SAMPLES:
            got = trace(r, o, d, s, k)
            same(got[ok], rc.record_of(paths, k)[ok], f"{what} set {which} samples {k}")
    assert np.any(rc.record_of(paths, 2)[ok, :3] != 0)


# ---- 1. parity with the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("name", rc.COMBO_NAMES)
def test_parity_with_the_oracle(oracle, name, strict):
    r = renderer(name)
    r.set_strict_traversal(strict)
    try:
        check_against_oracle(r, name, "shallow", f"{name} strict={strict}")
    finally:
        r.set_strict_traversal(False)


@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
def test_parity_on_the_deep_mesh(oracle, strict):
    """24-entry stacks: the class kernel, and the generic one in strict mode."""
    name = "cornell+mesh"
    r = renderer(name, "deep")
    assert 15 < r.bvh_info()[0] <= 23
    r.set_strict_traversal(strict)
    try:
        check_against_oracle(r, name, "deep", f"deep {name} strict={strict}")
    finally:
        r.set_strict_traversal(False)


@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("name", rc.SHADING_NAMES)
def test_parity_on_shading_scenes(oracle, name, strict):
    """Maps of odd shapes, zero tangents, the example sphere with maps, and a
    scene with NaN normals (tests/shading_cases.py): the vr_radiance_* kernels
    are instantiations of their own of the shading code, which saw 32 x 32 maps only."""
    import shading_cases as sh
    key = ("shading", name)
    if key not in _live:
        _live[key] = VRendererHIP(0)
        scenes.load_into(_live[key], sh.make_case(name))
    r = _live[key]
    r.set_strict_traversal(strict)
    try:
        for which in ("A", "B"):
            o, d, s = rc.ray_set(which)
            paths, ok = rc.shading_reference(name, which)
            for k in rc.SHADING_SAMPLES:
                got, want = trace(r, o, d, s, k), rc.record_of(paths, k)
                what = f"{name} strict={strict} set {which} samples {k}"
                if name in sh.NAN_CASES:
                    assert ok.all() and not np.isnan(got[:, 3]).any(), what
                    bad = np.flatnonzero(~rc.same_or_nan_in_both(got, want))
                    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ (first {bad[:5].tolist()}: " \
                                          f"{got[bad[:2]].tolist()} against {want[bad[:2]].tolist()})"
                else:
                    same(got[ok], want[ok], what)
    finally:
        r.set_strict_traversal(False)


# ---- 2. parity with the renderer, independent of the oracle -------------------------------------
@pytest.mark.parametrize("name", rc.COMBO_NAMES)
def test_parity_with_the_renderer(name):
    r = renderer(name)
    sc = fl.scene_of(rc.combo_of(name))
    t = 40503
    r.clearBuffer()
    r.render(frames=1, times=[t])
    accum, depth = r.read_accum(), r.read_depth8()
    d = rc.camera_dirs(sc)
    o = np.tile(np.asarray(sc["camera"]["origin"], np.float32), (len(d), 1))
    got = trace(r, o, d, rc.camera_seeds(sc, time=t), 2).reshape(fl.H, fl.W, 4)
    assert (rc.u32(got[..., :3]) == rc.u32(accum[..., :3])).all(), name
    assert (rc.depth_byte(got[..., 3]) == depth[..., 0]).all(), name
    assert np.any(accum[..., :3] != 0)
    r.clearBuffer()


# ---- 3. ray counts and the grid-stride loop ------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ray_counts(oracle, n):
    name = "cornell+mesh"
    o, d, s = rc.ray_set("A")
    paths, ok = rc.reference(name, "A")
    got = trace(renderer(name), o[:n], d[:n], s[:n], 2)
    same(got[ok[:n]], rc.record_of(paths, 2)[:n][ok[:n]], f"{n} rays")


def test_more_rays_than_a_resident_set(oracle):
    import torch
    name = "cornell+example"
    # the launcher's resident set: VR_SPHERE_MIN_WAVES (6) blocks of 256 rays on each CU
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (6 * cus + 3) * 256 + 77
    o, d, s = rc.ray_set("A")
    idx = np.arange(n) % len(o)
    got = trace(renderer(name), o[idx], d[idx], s[idx], 2)
    same(got, got[idx], "record i against record i mod 1024")
    paths, ok = rc.reference(name, "A")
    same(got[:len(o)][ok], rc.record_of(paths, 2)[ok], "the first 1,024 records")


# ---- 4. invalid rays -------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
def test_invalid_rays_in_a_batch(strict):
    r = renderer("cornell+mesh")
    o, d, s = (a[:200].copy() for a in rc.ray_set("B"))
    r.set_strict_traversal(strict)
    try:
        clean = trace(r, o, d, s, 2)
        rows = [0, 31, 63, 64]
        o[0, 1] = np.nan
        d[31, 2] = np.inf
        d[63] = 0.0
        d[64] = (3e19, -3e19, 3e19)                     # finite, the squared length overflows
        got = trace(r, o, d, s, 2)
    finally:
        r.set_strict_traversal(False)
    assert not rc.u32(got[rows]).any()                  # exactly {0, 0, 0, 0}
    rest = np.setdiff1d(np.arange(len(o)), rows)
    same(got[rest], clean[rest], "the valid rays of the batch")
    assert np.any(clean[rows] != 0)


# ---- 5. nothing else moves --------------------------------------------------------------------------
def test_a_call_leaves_everything_else_alone():
    name = "cornell+mesh"
    sc = fl.scene_of(rc.combo_of(name))
    o, d, s = rc.ray_set("B")
    state = {}
    for query in (False, True):
        q = VRendererHIP(0)
        scenes.load_into(q, sc)
        q.render(frames=2, times=[11, 12])
        before = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount(), q.export_mesh_flat())
        if query:
            a, b = trace(q, o, d, s, 2), trace(q, o, d, s, 2)
            same(a, b, "two calls")
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


# ---- 6. device meshes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,refit", [("cornell+mesh", False), ("mesh+tex_d+tex_n+tex_s", True)],
                         ids=["built", "refit"])
def test_device_meshes(oracle, name, refit):
    combo = rc.combo_of(name)
    sc = fl.scene_of(combo[:3] + (0,) + combo[4:])      # the mesh comes from the device build
    mesh = scenes.torus_knot(40, 20)
    o, d, s = (a[:256] for a in rc.ray_set("B"))
    q = VRendererHIP(0)
    scenes.load_into(q, sc)
    device_build(q, mesh, 2, "sah")
    if refit:
        q.refitMeshDevice(dev(deform(mesh["positions"])))
    flat = q.export_mesh_flat()
    got = trace(q, o, d, s, 2)
    q.cleanUp()
    paths = rc.oracle_paths(dict(sc, mesh_flat=flat), o, d, s, 2)
    ok = rc.kept(paths)
    same(got[ok], rc.record_of(paths, 2)[ok], f"device mesh {name} refit={refit}")
    assert np.isfinite(got[ok]).all() and np.any(got[ok, :3] != 0)


# ---- 7. sessions and refusals ------------------------------------------------------------------------------
def test_between_unsynchronised_renders_of_a_session(oracle):
    name = "cornell+mesh"
    sc = fl.scene_of(rc.combo_of(name))
    o, d, s = rc.ray_set("B")
    paths, ok = rc.reference(name, "B")
    images = {}
    for query in (False, True):
        q = VRendererHIP(0)
        scenes.load_into(q, sc)
        q.set_service(1)
        q.render(frames=2, times=[11, 12], sync=False)
        if query:
            s0 = q.service_info()["sessions"]
            got = trace(q, o, d, s, 2)
            same(got[ok], rc.record_of(paths, 2)[ok], "inside a session")
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


def test_refusals():
    import torch
    o, d, s = (dev(a[:64], t) for a, t in zip(rc.ray_set("B"), (np.float32, np.float32, np.uint32)))
    q = VRendererHIP([0])                                # a multi-device context of one device
    q.init(64, 48)
    with pytest.raises(VRHIPError) as e:
        q.traceRadiance(o, d, s)
    assert e.value.code == -1 and "multi-device" in str(e.value)
    q.cleanUp()
    q = fresh()                                          # HDRI mode, no environment
    with pytest.raises(VRHIPError) as e:
        q.traceRadiance(o, d, s)
    assert e.value.code == -3
    assert tuple(q.traceRadiance(o[:0], d[:0], s[:0]).shape) == (0, 4)      # nothing to do comes first, as in vrhip_render
    q.useCornellBox(True)                                # a scene without a mesh
    want = q.traceRadiance(o, d, s).cpu().numpy()
    assert np.isfinite(want).all() and np.any(want[:, :3] != 0)
    for samples in (0, 4097):
        with pytest.raises(VRHIPError) as e:
            q.traceRadiance(o, d, s, samples=samples)
        assert e.value.code == -1
    p = lambda x: ctypes.c_void_p(x.data_ptr())                            # noqa: E731
    out = torch.zeros((65, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert q._lib.vrhip_trace_radiance(q._ctx, p(o), p(d), p(s), 64, 2, ctypes.c_void_p(out.data_ptr() + 4)) == -1
    assert q._lib.vrhip_trace_radiance(q._ctx, p(o), p(d), None, 64, 2, p(out)) == -1
    assert not out.cpu().numpy().any()
    assert q._lib.vrhip_trace_radiance(q._ctx, None, None, None, 0, 2, None) == 0
    wrong = [dict(origins=o.cpu(), dirs=d), dict(origins=o, dirs=d.double()), dict(origins=o, dirs=d[:-1]),
             dict(origins=o[:, :2].contiguous(), dirs=d), dict(origins=o, dirs=d, seeds=s[:-1]),
             dict(origins=o, dirs=d, seeds=s.float()), dict(origins=o, dirs=d, seeds=s[:, :1].contiguous()),
             dict(origins=o, dirs=d, seeds=s.cpu()), dict(origins=None, dirs=d), dict(origins=o, dirs=None)]
    for kw in wrong:                                     # device, dtype, shape, missing
        with pytest.raises(ValueError):
            q.traceRadiance(**kw)
    drawn = q.traceRadiance(o, d, samples=4)             # seeds drawn on the device
    assert tuple(drawn.shape) == (64, 4) and np.isfinite(drawn.cpu().numpy()).all()
    again = q.traceRadiance(o, d, s).cpu().numpy()
    assert (rc.u32(again) == rc.u32(want)).all()
    assert q.traceRadiance(o, d, s, samples=4096).shape[0] == 64           # the upper bound itself
    q.cleanUp()
