"""The HIP kernels on the scalars a launch carries by value
(tests/launch_scalar_cases.py): time seeds of 2^24 and more, frame numbers
past 65,536, cameras at the poles, inside spheres, far away, with scaled,
skewed, long and left-handed bases and fov_scale from 0 to 1e3, Fresnel pairs
at the edges of pow, and images of one tile column, one tile row, the widest
the ABI takes and no tile at all -- against the portable-libm oracle, bit for
bit: accumulation as uint32, RGBA8 and depth8 as bytes, on the rendered region.
What each case would catch is measured in tests/test_launch_scalars_cpu.py; the
fixtures of eight of them, rendered by the reference itself, are compared in
tests/test_reference_fixtures.py.

Every render asserts vrhip_last_launch_info: render_kernel for the sphere
scenes, path_pool for mesh launches, path_pool_graph for synchronous one-frame
calls of a context created under VRHIP_GRAPH=1 with kernel timing off, service
for unsynchronised one-frame calls after set_service(1).

Where the pixel seeds s1 = x * frame and s2 = y * time are formed, and the
tests that fail when that site alone keeps 24 bits of the time (T) or 16 bits
of the frame number (F) -- run once on an MI355X with a scratch build in which
an environment variable selected the site; with none selected all pass:
  render_kernel, s2 (T)                  test_time_seeds[C1-plain], test_long_accumulation[C1-launches]
  render_kernel, s1 (F)                  test_long_accumulation[C1-launches]
  path pool, start() of wave_body (T)    test_time_seeds[C2-multi_frame, -one_frame, -graph, -tiled, -time_seed],
                                         the same five of C3, [C2D-plain], test_long_accumulation[C2-launches]
  path pool, start() of wave_body (F)    test_long_accumulation[C2-launches]
  service, descriptor loads (T) / (F)    test_time_seeds[C2-service], [C3-service],
                                         test_long_accumulation[C2-service] / the last alone
  service, the multiply in start() (T)   test_time_seeds[C2-service], [C3-service], test_long_accumulation[C2-service]
  host, RenderParams::times of a launch  every test_time_seeds case but the two service ones, and
  (launch_decisions) (T)                 test_long_accumulation[C1-launches], [C2-launches]
  host, the service descriptor's times   test_time_seeds[C2-service], [C3-service],
  (svc_post) (T)                         test_long_accumulation[C2-service]
A time kept to 24 bits makes frame_times(2^24 + 1) render as frame_times(1),
which differs on 96 % of the pixels below row 0 (tests/test_launch_scalars_cpu.py).

Measured on one MI355X (16 host CPUs), per test, oracle renders included:
  test_time_seeds         0.01 to 0.36 s (C3-multi_frame; the first test also loads the libraries, 1.6 s)
  test_long_accumulation  C1-launches 2.4 s (1,025 calls 0.06 s, the per-pixel expectation 2.3 s), C2-launches 4.0 s
                          (0.30 s and 3.7 s), C2-service 0.04 s (0.03 s; the expectation is shared with C2-launches)
  test_cameras            0.01 to 0.14 s (C4), 15 to 30 renders each
  test_fresnel_pairs      0.03 to 0.09 s, 29 to 60 renders each
  test_image_shapes       0.00 to 0.50 s (65535x16 C3, two frames and six tiled ranks; 65535x16 C2 0.34 s)
  test_image_without_a_whole_tile  0.00 to 0.24 s
  the module, 45 tests    12 s
"""
import os
import time

import numpy as np
import pytest

import launch_scalar_cases as lc
import pyoracle as po

pytestmark = pytest.mark.gpu

ROUTE_KIND = {"multi_frame": "path_pool", "one_frame": "path_pool", "graph": "path_pool_graph", "service": "service",
              "tiled": "path_pool", "time_seed": "path_pool"}


# ---- contexts, launches, comparison ------------------------------------------------------
def loaded(sc, graph=False):
    """A context with the scene loaded; graph: created under VRHIP_GRAPH=1
    (vrhip_create reads it), kernel timing off as the one-frame graph needs."""
    from vrenderer_pathtracer_amd import VRendererHIP, scenes
    r = VRendererHIP(0)
    old = os.environ.get("VRHIP_GRAPH")
    os.environ["VRHIP_GRAPH"] = "1" if graph else "0"
    try:
        scenes.load_into(r, sc)
    finally:
        if old is None:
            del os.environ["VRHIP_GRAPH"]
        else:
            os.environ["VRHIP_GRAPH"] = old
    if graph:
        r.set_kernel_timing(False)
    return r


def launch(r, route, times):
    """Clear, render `times` by a route, synchronise; returns the launch kind reported."""
    r.clearBuffer()
    if route in ("plain", "multi_frame", "tiled"):
        r.render(frames=len(times), times=list(times))
    elif route == "time_seed":                           # times = NULL: every frame carries time_seed
        assert len(set(times)) == 1
        r.render(frames=len(times), times=None, time_seed=times[0])
    elif route in ("one_frame", "graph"):                # synchronous one-frame calls: inline primary pass
        for t in times:
            r.render(frames=1, times=[t])
    elif route == "service":                             # unsynchronised one-frame calls: one session
        for t in times:
            r.render(frames=1, times=[t], sync=False)
        r.sync()
    else:
        raise ValueError(route)
    return r.last_launch_info()["kind"]


def images(r):
    return r.read_accum(), r.read_rgba8(), r.read_depth8()


def differences(got, want, where, mask=None):
    """Failure lines of (accum, rgba8, depth8) against the oracle's on the
    rendered region; mask: the pixels compared (all by default), and then the
    accumulation outside it must be zero."""
    out = []
    if np.isnan(got[0]).any():
        out.append(f"{where} accum: NaNs in a case that has none")
    for what, g, w in zip(("accum", "rgba8", "depth8"), got, want):
        d = lc.differing(lc.region(g), lc.region(w))
        if mask is not None:
            d = d & lc.region(mask)
        if d.any():
            y, x = np.argwhere(d)[0]
            out.append(f"{where} {what}: {int(d.sum())} pixels differ, first at x={x} y={y}: "
                       f"{g[y, x].tolist()} for {w[y, x].tolist()}")
    if mask is not None and got[0][~mask].any():
        out.append(f"{where}: accumulation on pixels of another rank")
    return out


def report(what, failures, t0, n):
    print(f"{what}: {n} renders in {time.perf_counter() - t0:.2f} s")
    if failures:
        pytest.fail(f"{what}: {len(failures)} differences from the oracle:\n" + "\n".join(failures[:40]), pytrace=False)


# ---- 1. time seeds ----------------------------------------------------------------------------
@pytest.mark.parametrize("scene,route", [(s, r) for s in lc.SEED_SCENES for r in lc.SEED_ROUTES[s]])
def test_time_seeds(native, oracle, scene, route):
    """One context per (scene, route) walks every time of SEED_TIMES, two
    frames each, and one call whose two frames carry the same time."""
    t0 = time.perf_counter()
    walk = lc.SEED_WALK_TIME_SEED if route == "time_seed" else lc.SEED_WALK
    kind = ROUTE_KIND.get(route, lc.LAUNCH_KIND[scene])
    own = lc.owned_mask(lc.W, lc.H, 0, 2) if route == "tiled" else None
    failures = []
    r = loaded(lc.scene_of(scene), graph=route == "graph")
    try:
        if route == "service":
            r.set_service(1)
        if route == "tiled":
            r.set_tiling(0, 2)
        for step, times in walk:
            got_kind = launch(r, route, times)
            where = f"{scene} {route} {step}"
            if got_kind != kind:
                failures.append(f"{where}: launched as {got_kind}, meant for {kind}")
            if r.getFrameCount() != len(times):
                failures.append(f"{where}: frame count {r.getFrameCount()}")
            failures += differences(images(r), lc.oracle_render(scene, times), where, own)
        if route == "service":
            assert r.service_info()["served"] == 2 * len(walk)
    finally:
        r.cleanUp()
    report(f"{scene} {route} ({lc.KERNEL[scene]})", failures, t0, len(walk))


# ---- 2. long accumulations ------------------------------------------------------------------------
@pytest.mark.parametrize("scene,route", [("C1", "launches"), ("C2", "launches"), ("C2", "service")])
def test_long_accumulation(native, oracle, scene, route):
    """65,600 frames on a 16 x 16 image in calls of 64: synchronous calls
    (render_kernel, the path pool) or one unsynchronised stream of calls after
    set_service(1).  The accumulation of LONG_PIXELS equals the sum of the
    oracle's per-sample results over every frame; the frame count is 65,600;
    and the last call, frames 65,537 to 65,600, equals the oracle continuing
    from the accumulation read back after frame 65,536, on every pixel."""
    sc = lc.long_scene(scene)
    calls = lc.LONG_FRAMES // lc.LONG_CALL
    times = [lc.long_time(f) for f in range(1, lc.LONG_FRAMES + 1)]
    kind = "service" if route == "service" else lc.LAUNCH_KIND[scene]
    t0 = time.perf_counter()
    r = loaded(sc)
    try:
        if route == "service":
            r.set_service(1)
        kinds = set()
        for c in range(calls - 1):
            r.render(frames=lc.LONG_CALL, times=times[c * lc.LONG_CALL:(c + 1) * lc.LONG_CALL], sync=route != "service")
            kinds.add(r.last_launch_info()["kind"])
        r.sync()
        assert r.getFrameCount() == lc.LONG_FRAMES - lc.LONG_CALL == 65536
        before = r.read_accum()
        r.render(frames=lc.LONG_CALL, times=times[-lc.LONG_CALL:], sync=route != "service")
        kinds.add(r.last_launch_info()["kind"])
        r.sync()
        frames, got = r.getFrameCount(), images(r)
    finally:
        r.cleanUp()
    t_gpu = time.perf_counter() - t0
    want = lc.long_expectation(scene)
    print(f"{scene} {route}: {calls} calls in {t_gpu:.2f} s, the expectation in {time.perf_counter() - t0 - t_gpu:.2f} s")
    assert kinds == {kind}, kinds
    assert frames == lc.LONG_FRAMES
    failures = []
    for (x, y), v in want.items():
        if got[0][y, x].tobytes() != v.tobytes():
            failures.append(f"pixel ({x}, {y}): {got[0][y, x].tolist()} for {v.tolist()}")
    cont = po.render(sc, frames=lc.LONG_CALL, times=times[-lc.LONG_CALL:], first_frame=lc.LONG_FRAMES - lc.LONG_CALL + 1,
                     libm=po.LIBM_PORTABLE, accum=before.copy())[:3]
    failures += differences(got, cont, f"{scene} {route} frames 65,537 to 65,600")
    if failures:
        pytest.fail(f"{scene} {route}: " + "\n".join(failures), pytrace=False)


# ---- 3. camera -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", lc.CAMERA_SCENES)
def test_cameras(native, oracle, scene):
    """One context per scene walks its cameras: the mesh scenes by a
    two-frame launch and by synchronous one-frame calls, the sphere scenes by
    a two-frame launch."""
    from vrenderer_pathtracer_amd.renderer import Camera
    t0 = time.perf_counter()
    routes = ("multi_frame", "one_frame") if lc.LAUNCH_KIND[scene] == "path_pool" else ("plain",)
    failures, n = [], 0
    r = loaded(lc.scene_of(scene))
    try:
        for name in lc.cameras_on(scene):
            cam = lc.camera_of(name)
            r.setCamera(Camera(cam["origin"], cam["dir"], cam["up"], cam["right"], cam["fov_scale"]))
            want = lc.oracle_render(scene, camera=name)
            for route in routes:
                got_kind = launch(r, route, lc.DEFAULT_TIMES)
                n += 1
                where = f"{scene} {name} {route}"
                if got_kind != lc.LAUNCH_KIND[scene]:
                    failures.append(f"{where}: launched as {got_kind}")
                failures += differences(images(r), want, where)
    finally:
        r.cleanUp()
    report(f"{scene} cameras", failures, t0, n)


# ---- 4. Fresnel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", lc.FRESNEL_SCENES)
def test_fresnel_pairs(native, oracle, scene):
    """One context per scene walks the pairs; no pair makes a NaN on the
    oracle (tests/test_launch_scalars_cpu.py), so every pixel compares bit for bit."""
    t0 = time.perf_counter()
    routes = ("multi_frame", "one_frame") if lc.LAUNCH_KIND[scene] == "path_pool" else ("plain",)
    failures, n = [], 0
    r = loaded(lc.scene_of(scene))
    try:
        for coef, power in lc.fresnel_on(scene):
            r.m_fresnelCoef = coef
            r.setFresnelPower(power)
            want = lc.oracle_render(scene, fresnel=(coef, power))
            assert not np.isnan(want[0]).any()
            for route in routes:
                got_kind = launch(r, route, lc.DEFAULT_TIMES)
                n += 1
                where = f"{scene} Fresnel ({coef}, {power}) {route}"
                if got_kind != lc.LAUNCH_KIND[scene]:
                    failures.append(f"{where}: launched as {got_kind}")
                failures += differences(images(r), want, where)
    finally:
        r.cleanUp()
    report(f"{scene} Fresnel pairs", failures, t0, n)


# ---- 5. image shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,scene,frames", [(sz, s, f) for sz, runs in lc.SHAPES.items() for s, f in runs],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_image_shapes(native, oracle, size, scene, frames):
    """One frame: a synchronous one-frame call (the kernels that trace the
    camera ray themselves, its pixel packed as x << 16 | y); two frames: one
    launch behind a primary pass.  Then, on the single tile column, the single
    tile row and the widest image, ranks 0 and n - 1 of 2, 3 and 7: the owned
    pixels (vrhip_tile_pixels) equal the oracle, the others stay zero."""
    w, h = size
    t0 = time.perf_counter()
    times = lc.shape_times(frames)
    route = "one_frame" if frames == 1 else "multi_frame"
    want = lc.oracle_render(scene, times, w=w, h=h)
    failures, n = [], 1
    r = loaded(lc.scene_of(scene, w, h))
    try:
        kind = launch(r, route, times)
        assert kind == "path_pool" and r.getFrameCount() == frames
        assert r.owned_pixels() == (w // 16) * (h // 16) * 256
        got = images(r)
        failures += differences(got, want, f"{w}x{h} {scene} {route}")
        # nothing is written outside the rendered region
        rows, cols = (h // 16) * 16, (w // 16) * 16
        for a in got:
            assert not a[rows:].any() and not a[:, cols:].any()
        for rank, n_ranks in (lc.TILINGS if size in lc.TILED_SHAPES else ()):
            own = lc.owned_mask(w, h, rank, n_ranks)
            r.set_tiling(rank, n_ranks)
            kind = launch(r, route, times)
            n += 1
            assert kind == "path_pool" and r.owned_pixels() == int(own.sum())
            failures += differences(images(r), want, f"{w}x{h} {scene} {route} rank {rank} of {n_ranks}", own)
    finally:
        r.cleanUp()
    report(f"{w}x{h} {scene} {frames} frame(s)", failures, t0, n)


@pytest.mark.parametrize("scene", ["C1", "C2", "C3"])
def test_image_without_a_whole_tile(native, scene):
    """15 x 40 holds no 16 x 16 tile.  vrhip_create takes it (1 to 65,535
    pixels per side) and vrhip_render launches nothing (launch_render and
    launch_finish return at once for no tiles): the frame count advances over
    buffers that stay zero, on every route, and no service session opens.
    The same under VRHIP_GRAPH=1 on the mesh scenes, and for a tiled rank that
    owns no tile (this case found the one-frame graph refusing such a call)."""
    from vrenderer_pathtracer_amd import VRHIPError, VRendererHIP
    w, h = lc.NO_TILE_SHAPE
    r = loaded(lc.scene_of(scene, w, h))
    try:
        assert r.owned_pixels() == 0
        r.render(frames=2, times=list(lc.DEFAULT_TIMES))
        assert r.getFrameCount() == 2
        r.render(frames=1, times=[7])
        r.set_service(1)
        for t in (8, 9):
            r.render(frames=1, times=[t], sync=False)
        r.sync()
        assert r.getFrameCount() == 5 and r.service_info()["served"] == 0
        for a in images(r):
            assert not a.any()
        r.clearBuffer()
        assert r.getFrameCount() == 0
    finally:
        r.cleanUp()
    if lc.LAUNCH_KIND[scene] == "path_pool":
        # under VRHIP_GRAPH=1 a one-frame call without a tile has no kernel node to capture: it was refused with
        # "one-frame graph: expected the path kernel and the finish pass" until launch_decisions left such launches
        # off the graph; likewise rank 1 of 2 of a one-tile image
        for size, tiling in ((lc.NO_TILE_SHAPE, None), ((17, 16), (1, 2))):
            r = loaded(lc.scene_of(scene, *size), graph=True)
            try:
                if tiling:
                    r.set_tiling(*tiling)
                assert r.owned_pixels() == 0
                for t in (7, 8):
                    r.render(frames=1, times=[t])
                assert r.getFrameCount() == 2 and r.last_launch_info()["kind"] == "path_pool"
                for a in images(r):
                    assert not a.any()
            finally:
                r.cleanUp()
    # the limits of vrhip_create: a side of 0 or of more than 65,535 pixels is refused with a text
    for bad in ((0, 16), (16, 0), (lc.MAX_WIDTH + 1, 16), (16, lc.MAX_WIDTH + 1)):
        with pytest.raises(VRHIPError, match="1..65535 pixels per side"):
            VRendererHIP(0).init(*bad) if bad[0] and bad[1] else _create(*bad)


def _create(w, h):
    """vrhip_create itself (VRendererHIP.init asserts non-zero sides first)."""
    import ctypes
    from vrenderer_pathtracer_amd import _native
    ctx = ctypes.c_void_p(None)
    _native.check(_native.lib().vrhip_create(0, w, h, ctypes.byref(ctx)), "vrhip_create")
