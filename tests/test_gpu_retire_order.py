"""Retire-first order of the Cornell-box mesh path kernels (vr_kernel.hpp
retire_first): a lane takes the short exits of its ended path (escape, last
bounce) and starts the next path in the same wave BEFORE the shading pass.
That only happens in waves that take more than one chunk, i.e. when the launch
holds more paths than the resident set has lanes (256 CUs x 28 waves x 64 =
458,752): 192x160 at 32 frames is 1.97 M paths, about four per lane.  Every
launch kind that runs such a kernel is compared with the portable-libm oracle
bit for bit (accumulation, RGBA8, depth); the oracle renders once per scene.
"""
import numpy as np
import pytest

import pyoracle as po
from vrenderer_pathtracer_amd import VRendererHIP, scenes
from vrenderer_pathtracer_amd.tiles import owned_pixels

pytestmark = pytest.mark.gpu

W, H = 192, 160
FRAMES = 32


def _times(sc, n):
    return [sc["time"] + k for k in range(n)]


@pytest.fixture(scope="module")
def c2_ref(oracle):
    sc = scenes.make_scene("C2", W, H)
    oa, orgba, od, _ = oracle.render(sc, frames=FRAMES, times=_times(sc, FRAMES), libm=po.LIBM_PORTABLE)
    for a in (oa, orgba, od):
        a.setflags(write=False)
    return sc, (oa, orgba, od)


def _run(sc, calls, service, tiling=None):
    """Async render calls of `calls` frames each; accum, RGBA8, depth and the launch kinds."""
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.set_service(service)
    if tiling:
        r.set_tiling(*tiling)
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


def _bitexact(got, ref, pix=None):
    """Equal bit for bit on the rendered area (whole 16x16 tiles), or on the flat pixel list `pix`."""
    for g, o, what in zip(got, ref, ("accum", "rgba8", "depth8")):
        if pix is None:
            g, o = g[:H // 16 * 16, :W // 16 * 16].reshape(-1, 4), o[:H // 16 * 16, :W // 16 * 16].reshape(-1, 4)
        else:
            g, o = g.reshape(-1, 4)[pix], o.reshape(-1, 4)[pix]
        if g.dtype == np.float32:
            g, o = g.view(np.uint32), o.view(np.uint32)
        bad = int((g != o).any(-1).sum())
        assert bad == 0, f"{what}: {bad} of {len(g)} pixels differ from the oracle"


def test_session_retires_into_next_launch(native, c2_ref):
    """Two back-to-back 16-frame calls in one service session: lanes retire
    paths of launch L while starting paths of launch L + 1."""
    sc, ref = c2_ref
    got, kinds = _run(sc, [16, 16], service=1)
    assert kinds == ["service", "service"]
    assert np.any(ref[0][..., :3] != 0)
    _bitexact(got, ref)


def test_launch_by_launch(native, c2_ref):
    """The same frames launch by launch: the whole-frame kernel."""
    sc, ref = c2_ref
    got, kinds = _run(sc, [16, 16], service=0)
    assert kinds == ["path_pool", "path_pool"]
    _bitexact(got, ref)


def test_tiled_rank_single_launch(native, c2_ref):
    """One 32-frame launch on rank 1 of 3 (the shard launch shape), compared
    on the tiles the rank owns; nothing is written outside them."""
    sc, ref = c2_ref
    got, kinds = _run(sc, [FRAMES], service=0, tiling=(1, 3))
    assert kinds == ["path_pool"]
    pix = owned_pixels(W, H, 1, 3)
    assert 0 < len(pix) < W * H
    _bitexact(got, ref, pix)
    other = np.ones(W * H, bool)
    other[pix] = False
    assert np.all(got[0].reshape(-1, 4)[other] == 0)


@pytest.fixture(scope="module")
def c2d_ref(oracle):
    sc = scenes.make_scene("C2D", W, H)
    ref = oracle.render(sc, frames=16, times=_times(sc, 16), libm=po.LIBM_PORTABLE)[:3]
    for a in ref:
        a.setflags(write=False)
    return sc, ref


@pytest.mark.parametrize("service", [1, 0])
def test_cornell_mesh_class_kernel(native, c2d_ref, service):
    """The Cornell mesh feature-class kernel (C2D: a diffuse map), one
    16-frame call in a session and as a plain launch."""
    sc, ref = c2d_ref
    got, kinds = _run(sc, [16], service=service)
    assert kinds == ["service" if service else "path_pool"]
    _bitexact(got, ref)
