"""The straight-line sphere tests and their single range vote
(vr_kernel.hpp intersect_spheres, sphere_tail; vr_math.hpp sphere_root) on
rays crafted for them, through vrhip_trace_radiance, which shares the code
with the render kernels -- against the oracle's trace, bit for bit -- and two
small C2-class renders against the oracle by SHA-256.

The 2,048 rays: tangents to the two small spheres and the light whose
discriminant is exactly 0 in fp32 (axis-parallel, so every term is exact) and
a few ulps either side of it; origins 0.05 off every wall next to every edge
and corner of the box; axis-parallel rays; rays with one or two zero
direction components.  Zero components are +0: the yardstick's camera sum
turns a -0 into +0 (tests/radiance_cases.py).
"""
import functools
import hashlib

import numpy as np
import pytest

import flag_lattice as fl
import radiance_cases as rc
from vrenderer_pathtracer_amd import VRendererHIP, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
N_RAYS = 2048
SCENES = {"no mesh": "cornell", "shallow mesh": "cornell+mesh"}
# (centre, radius): vr_kernel.hpp small_sphere, cornell_sphere(0)
SMALL0, SMALL1, LIGHT = ((15.0, 0.0, 15.0), 3.5), ((25.0, 0.0, 15.0), 3.5), ((0.0, 209.0, 0.0), 160.0)
WALLS = dict(x=(-50.0, 50.0), y=(-50.0, 50.0), z=(-100.0,))       # the box is open towards +z


def step(x, k):
    """x moved k floats up (k < 0: down)."""
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


def det_of(o, d, sphere):
    """Sphere::intersect's discriminant in fp32, in its operation order, for a unit axis direction."""
    c, r = np.asarray(sphere[0], f32), f32(sphere[1])
    op = c - np.asarray(o, f32)
    b = (op[0] * d[0] + op[1] * d[1]) + op[2] * d[2]
    return f32(f32(b * b - ((op[0] * op[0] + op[1] * op[1]) + op[2] * op[2])) + r * r)


def tangents():
    """Axis-parallel rays touching a sphere: the line is r away from the
    centre along one axis and the ray starts 20 before the touching point.
    The offset coordinate is then moved by 0, +-1 ... +-64 floats."""
    rays, dets = [], []
    for sphere in (SMALL0, SMALL1, LIGHT):
        c, r = sphere
        for along in range(3):
            for side in range(3):
                if side == along:
                    continue
                for sgn in ((-1.0,) if sphere is LIGHT else (-1.0, 1.0)):      # the light: its underside only
                    if sphere is LIGHT and side != 1:
                        continue
                    for k in (0, 1, -1, 2, -2, 4, -4, 8, -8, 16, -16, 64, -64):
                        o = np.array(c, f32)
                        o[side] = step(f32(c[side]) + f32(sgn * r), k)
                        o[along] = f32(c[along] - 20.0)
                        d = np.zeros(3, f32)
                        d[along] = 1.0
                        rays.append((o, d))
                        dets.append(det_of(o, d, sphere))
    return rays, np.array(dets, f32)


def wall_origins():
    """0.05 off a wall, at every edge and corner and at the middle of every
    face: each coordinate is at either wall of its axis or in between."""
    xs = (-49.95, 3.7, 49.95)
    ys = (-49.95, 2.1, 49.95)
    zs = (-99.95, -31.3, 40.0)
    pts = [(x, y, z) for x in xs for y in ys for z in zs if (x, y, z) != (xs[1], ys[1], zs[1]) and
           (abs(x) > 49 or abs(y) > 49 or z < -99)]
    return np.array(pts, f32)


@functools.lru_cache(maxsize=None)
def crafted():
    """(origins, dirs, seeds, dets of the tangent rays), never written."""
    rng = np.random.default_rng(8128)
    o, d = [], []
    tan, dets = tangents()
    for a, b in tan:
        o.append(a); d.append(b)
    n_tan = len(o)
    # off the walls: towards the wall, along it, and away, plus random directions
    for p in wall_origins():
        for _ in range(16):
            v = rng.normal(0.0, 1.0, 3)
            o.append(p); d.append((v / np.linalg.norm(v)).astype(f32))
        for ax in range(3):
            for s in (-1.0, 1.0):
                v = np.zeros(3, f32)
                v[ax] = s
                o.append(p); d.append(v)
    # axis-parallel rays from inside the box
    for p in rng.uniform((-45, -45, -95), (45, 45, 60), (40, 3)).astype(f32):
        for ax in range(3):
            for s in (-1.0, 1.0):
                v = np.zeros(3, f32)
                v[ax] = s
                o.append(p); d.append(v)
    # one or two zero components (the second kind are axis-parallel again, of any length)
    while len(o) < N_RAYS:
        p = rng.uniform((-45, -45, -95), (45, 45, 60)).astype(f32)
        v = (rng.normal(0.0, 1.0, 3) * rng.uniform(0.1, 10.0)).astype(f32)
        v[rng.integers(0, 3)] = 0.0
        if len(o) % 5 == 0:
            v[rng.integers(0, 3)] = 0.0
        if not v.any():
            continue
        o.append(p); d.append(v)
    o, d = np.array(o[:N_RAYS], f32), np.array(d[:N_RAYS], f32)
    d = np.where(d == 0, f32(0.0), d)                                  # +0, never -0
    s = rng.integers(0, 2**32, (N_RAYS, 2), dtype=np.uint64).astype(np.uint32)
    assert n_tan < N_RAYS and not np.signbit(d[d == 0]).any()
    out = (np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(s), dets)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(scene_name):
    """The oracle's two paths per crafted ray in one scene: computed once, shared, never written."""
    import pyoracle as po
    po.build()
    o, d, s, _ = crafted()
    paths = rc.oracle_paths(fl.scene_of(rc.combo_of(SCENES[scene_name])), o, d, s, 2)
    paths.setflags(write=False)
    return paths


_live = {}


def renderer(scene_name):
    if scene_name not in _live:
        r = VRendererHIP(0)
        scenes.load_into(r, fl.scene_of(rc.combo_of(SCENES[scene_name])))
        _live[scene_name] = r
    return _live[scene_name]


@pytest.fixture(scope="module", autouse=True)
def _renderers(native):
    yield
    for r in _live.values():
        r.cleanUp()
    _live.clear()


def dev(a, dtype=np.float32):
    import torch
    a = np.array(a, dtype=dtype, order="C")
    if dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda(0)


def test_the_crafted_rays_are_what_they_claim():
    o, d, s, dets = crafted()
    assert len(o) == N_RAYS
    # tangents: exactly 0 for every unmoved ray, and both signs within a few ulps of b * b
    assert (dets == 0).sum() >= 14 and (dets < 0).any() and (dets > 0).any()
    assert np.abs(dets).max() < 0.5
    axis = ((d != 0).sum(-1) == 1)
    assert axis.sum() > 400 and ((d == 0).sum(-1) == 1).sum() > 100
    w = wall_origins()
    assert len(w) == 25 and all(np.isin(f32(v), w[:, i]).all() for i, v in ((0, (-49.95, 49.95)), (1, (-49.95, 49.95)), (2, (-99.95,))))


@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("scene_name", list(SCENES))
def test_crafted_rays_against_the_oracle(oracle, scene_name, strict):
    o, d, s, _ = crafted()
    paths = reference(scene_name)
    assert np.isfinite(paths).all()
    r = renderer(scene_name)
    r.set_strict_traversal(strict)
    try:
        for k in (1, 2):
            got = r.traceRadiance(dev(o), dev(d), dev(s, np.uint32), samples=k).cpu().numpy()
            want = rc.record_of(paths, k)
            bad = np.flatnonzero((rc.u32(got) != rc.u32(want)).any(-1))
            assert len(bad) == 0, (f"{scene_name} strict={strict} samples={k}: {len(bad)} of {N_RAYS} records differ "
                                   f"(first {bad[:5].tolist()}: {got[bad[:2]].tolist()} against {want[bad[:2]].tolist()})")
    finally:
        r.set_strict_traversal(False)
    assert np.any(rc.record_of(paths, 2)[:, :3] != 0)


@pytest.mark.parametrize("frames", [1, 4], ids=["one frame", "4 frames of 2 paths"])
def test_c2_class_render_against_the_oracle(oracle, frames):
    sc = dict(fl.scene_of(rc.combo_of("cornell+mesh")), width=64, height=48)
    assert fl.kernel_of(rc.combo_of("cornell+mesh")) == "spec_c2"
    times = [fl.TIMES[0] + i for i in range(frames)]
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.render(frames=frames, times=times)
    got = r.read_accum()
    assert r.getFrameCount() == frames
    r.cleanUp()
    ref, _, _, _ = oracle.render(sc, frames=frames, times=times, libm=oracle.LIBM_PORTABLE)
    assert np.any(ref[..., :3] != 0)
    assert hashlib.sha256(np.ascontiguousarray(got, f32).tobytes()).hexdigest() == \
           hashlib.sha256(np.ascontiguousarray(ref, f32).tobytes()).hexdigest(), \
           f"{int((rc.u32(got) != rc.u32(ref)).any(-1).sum())} pixels differ from the oracle"
