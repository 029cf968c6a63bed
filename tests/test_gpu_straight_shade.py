"""The branch-free shading pass of the Cornell-box mesh path-pool kernels
(vr_kernel.hpp straight_shade): a hit's constants from its row of kHitTab, one
hit point and one normalisation for every hit kind.  The render service and the
launch-by-launch path pool run the new fill_hit; one frame per call runs the
one-frame kernel, which keeps the switch and the per-kind arms, so equal
images compare the two forms on the device.  All three are compared with the
portable-libm oracle bit for bit (accumulation, RGBA8, depth), the parity rule
of the other C2 tests.

192x160 at 32 frames is 1.97 M paths, about four per lane of the resident set
(test_gpu_retire_order.py): lanes of one wave then hold different hit kinds
and bounces in the same pass.  64x48 is less than one resident set.  C2D (a
diffuse map on the knot) and C2 with all three maps run the Cornell mesh class
kernel, whose mesh lanes fetch attributes and texels -- and, with a normal
map, take the mapped normal -- inside the new form's one mesh block.
"""
import numpy as np
import pytest

import pyoracle as po
from vrenderer_pathtracer_amd import VRendererHIP, scenes
from vrenderer_pathtracer_amd.renderer import SURF_CORNELL, SURF_MESH, SURF_SMALL

pytestmark = pytest.mark.gpu

# (width, height, frames per call of the multi-frame routes, scene)
SIZES = {"192x160": (192, 160, [16, 16], "C2"), "64x48": (64, 48, [4, 4], "C2"),
         "C2D-64x48": (64, 48, [4, 4], "C2D"), "maps-192x160": (192, 160, [8, 8], "maps")}
C2_SIZES = [k for k, v in SIZES.items() if v[3] == "C2"]


def _scene(cfg, w, h):
    if cfg != "maps":
        return scenes.make_scene(cfg, w, h)
    sc = scenes.make_scene("C2D", w, h)         # the Cornell box and the knot with all three maps
    sc.update(scenes.procedural_textures())
    return sc


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@pytest.fixture(scope="module")
def refs(oracle):
    """The oracle's images of every size, rendered once."""
    out = {}
    for key, (w, h, calls, cfg) in SIZES.items():
        sc = _scene(cfg, w, h)
        n = sum(calls)
        out[key] = sc, _frozen(oracle.render(sc, frames=n, times=[sc["time"] + k for k in range(n)],
                                             libm=po.LIBM_PORTABLE)[:3])
    return out


def _render(sc, calls, service):
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.set_service(service)
    t, kinds = sc["time"], []
    for n in calls:
        r.render(frames=n, times=[t + k for k in range(n)], sync=False)
        kinds.append(r.last_launch_info()["kind"])
        t += n
    r.sync()
    out = r.read_accum(), r.read_rgba8(), r.read_depth8()
    nf = r.getFrameCount()
    r.cleanUp()
    assert nf == sum(calls)
    return out, kinds


def _frame(sc):
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.render(frames=2, times=[sc["time"], sc["time"] + 1])
    out = r.read_accum(), r.read_rgba8(), r.read_depth8()
    r.cleanUp()
    return out


@pytest.fixture(scope="module")
def other_frames(native, oracle):
    """A C3 and a C1 frame taken before this module's first C2 session (routes
    asks for this fixture), with the oracle's images of the same frames."""
    out = {}
    for cfg in ("C3", "C1"):
        sc = scenes.make_scene(cfg, 64, 48)
        ref = _frozen(oracle.render(sc, frames=2, times=[sc["time"], sc["time"] + 1], libm=po.LIBM_PORTABLE)[:3])
        out[cfg] = sc, _frozen(_frame(sc)), ref
    return out


@pytest.fixture(scope="module")
def routes(native, refs, other_frames):
    """Every size through the three routes, rendered once."""
    out = {}
    for key, (w, h, calls, _) in SIZES.items():
        sc = refs[key][0]
        svc, kinds = _render(sc, calls, service=1)
        assert kinds == ["service"] * len(calls)
        pool, kinds = _render(sc, calls, service=0)
        assert kinds == ["path_pool"] * len(calls)
        one, _ = _render(sc, [1] * sum(calls), service=0)
        out[key] = {"service": _frozen(svc), "launches": _frozen(pool), "one_frame": _frozen(one)}
    return out


def _words(a, w, h):
    a = a[:h // 16 * 16, :w // 16 * 16].reshape(-1, 4)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32)


def _assert_equal(got, want, w, h, who):
    for g, o, what in zip(got, want, ("accum", "rgba8", "depth8")):
        g, o = _words(g, w, h), _words(o, w, h)
        bad = int((g != o).any(-1).sum())
        assert bad == 0, f"{what}: {bad} of {len(g)} pixels of {who} differ"


@pytest.mark.parametrize("size", list(SIZES))
def test_three_render_paths_agree(routes, size):
    w, h = SIZES[size][:2]
    got = routes[size]
    assert np.any(got["one_frame"][0][..., :3] != 0)
    _assert_equal(got["service"], got["one_frame"], w, h, "the service against one frame per call")
    _assert_equal(got["launches"], got["one_frame"], w, h, "launch by launch against one frame per call")


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("route", ["service", "launches", "one_frame"])
def test_oracle(routes, refs, size, route):
    w, h = SIZES[size][:2]
    assert np.any(refs[size][1][0][..., :3] != 0)
    _assert_equal(routes[size][route], refs[size][1], w, h, f"{route} against the oracle")


@pytest.mark.parametrize("size", C2_SIZES)
def test_every_hit_kind_is_shaded(native, refs, size):
    """The camera rays' first hits -- each is shaded at bounce 0 -- include the
    knot, the light, the five walls and both small spheres."""
    sc = refs[size][0]
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    o, d = r.cameraRays()
    s = r.traceSurface(o, d)
    kind, prim = s["kind"].cpu().numpy(), s["prim"].cpu().numpy()
    typ, col, em = s["type"].cpu().numpy(), s["color"].cpu().numpy(), s["emission"].cpu().numpy()
    r.cleanUp()
    assert (kind == SURF_MESH).any(), "no camera ray hits the knot"
    for i in range(6):
        assert ((kind == SURF_CORNELL) & (prim == i)).any(), f"no camera ray hits Cornell sphere {i}"
    for i in range(2):
        assert ((kind == SURF_SMALL) & (prim == i)).any(), f"no camera ray hits small sphere {i}"
    light = (kind == SURF_CORNELL) & (prim == 0)
    assert not col[light].any() and em[light].all(), "the light: colour 0, emitting"
    for i in (1, 2):
        wall = (kind == SURF_CORNELL) & (prim == i)
        assert em[wall].all() and col[wall].all(), "an emitting wall"
    mirror = (kind == SURF_SMALL) & (prim == 0)
    assert (typ[mirror] == 0).all() and (typ[~mirror & (kind != 0)] == 1).all(), "the mirror sphere alone is specular"


def test_other_kernels_after_a_c2_session(routes, other_frames, refs):
    """A C3 and a C1 frame, which run kernels of another LDS layout, give the
    same bits after the C2 sessions of this module (routes, and one more here)
    as before the first of them, and both are the oracle's."""
    _, kinds = _render(refs["64x48"][0], [4, 4], service=1)
    assert kinds == ["service", "service"]
    for cfg, (sc, before, ref) in other_frames.items():
        assert np.any(ref[0][..., :3] != 0)
        _assert_equal(before, ref, 64, 48, f"{cfg} before the sessions against the oracle")
        after = _frame(sc)
        _assert_equal(after, before, 64, 48, f"{cfg} after the sessions against before them")
        _assert_equal(after, ref, 64, 48, f"{cfg} after the sessions against the oracle")
