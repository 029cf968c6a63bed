"""What the launch-scalar cases (tests/launch_scalar_cases.py) pin, from the
oracle, tests/flag_lattice.py and the host-only tile dealing alone: no GPU, no
reference.

A case is worth its GPU time only if a kernel that treated the scalar wrongly
would render it differently.  That is measured here on the oracle, with the
measured figures (64 x 48, two frames, portable libm) beside each threshold.

Time seeds.  frame_times(t) against frame_times(t') for the t' a narrowed
multiply or descriptor field would turn t into; share of the pixels in rows
y >= 1 whose camera ray hits (an escaped ray draws no random number) whose
accumulation bits differ:

                      C1       C2       C3 (hits: 21.6 % of the image)   C2D
  2^24 + 1 vs 1       96.4 %   96.7 %   99.0 %                          96.7 %   at least 90 %
  2^32 - 1 vs 1       96.4 %   96.7 %   98.7 %                          96.7 %   at least 90 %
  2^31 vs 0           49.2 %   49.4 %   49.9 %   (the odd rows)         49.4 %   at least 45 %

Cameras.  Every case changes at least 96.8 % of the pixels against the default
camera except `far` on the HDRI scenes (C3 21.7 %, C4 2.3 %: the pixels the
default camera's rays hit; from 1e4 units every ray escapes); at least 1 % is
required.  Shares of camera rays that hit, where a case claims one:
C3 up 15.5 %, down 15.6 %, basis_x3 2.5 %, basis_third 50.7 %, fov_10 0.2 %
(some); sky, far, dir_x10, fov_1e-3, fov_1e3, fov_0: 0 (none: the knot's axis
is a hole); C4 up 2.3 %, down 2.2 %, basis_x3 0.3 %, basis_third 18.9 % (some);
in_example, dir_x10, fov_1e-3, fov_0: 100 % (all); sky, far, fov_10, fov_1e3: 0.

Fresnel.  No pair makes a NaN on C3, C2N or C1T (the cap is 5 % of the pixels).
Least change against (0.1, 3): C3 4.8 % and C2N 7.9 % at (-0.5, 1); C1T 1.1 %
at (2, -1), with (-0.5, 1) at 0.81 % dropped there; at least 1 % is required.
"""
import ctypes

import numpy as np
import pytest

import launch_scalar_cases as lc
import pyoracle as po
import ref_cases as rc


def test_case_set_shape():
    assert (lc.W, lc.H) == (rc.W, rc.H) == (64, 48) and lc.KNOT == (24, 12)
    assert list(lc.DEFAULT_TIMES) == rc.times_of("C2")
    assert lc.SEED_TIMES == (0, 1, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 1, 0x9E3779B9)
    assert set(lc.SEED_ROUTES) == set(lc.SEED_SCENES) == {"C1", "C2", "C3", "C2D"}
    for scene in ("C2", "C3"):
        assert set(lc.SEED_ROUTES[scene]) == {"multi_frame", "one_frame", "graph", "service", "tiled", "time_seed"}
    # every time is walked; one step repeats a value; the time_seed form carries one value on every frame
    assert {ts[0] for _, ts in lc.SEED_WALK} == set(lc.SEED_TIMES)
    assert sum(ts[0] == ts[1] for _, ts in lc.SEED_WALK) == 1
    assert all(ts[0] != ts[1] for _, ts in lc.SEED_WALK[:-1])
    assert [ts for _, ts in lc.SEED_WALK_TIME_SEED] == [(t, t) for t in lc.SEED_TIMES]
    assert all(0 <= t < 2 ** 32 for _, ts in lc.SEED_WALK for t in ts)
    assert {t for t, _, _, _ in lc.SEED_PAIRS} <= set(lc.SEED_TIMES)
    assert lc.LONG_FRAMES > 65536 and lc.LONG_FRAMES % lc.LONG_CALL == 0 and lc.LONG_CALL == 64
    assert len(lc.LONG_PIXELS) >= 8 and {(0, 0), (15, 0), (0, 15), (15, 15)} <= set(lc.LONG_PIXELS)
    assert lc.long_time(1) < 2 ** 24 < lc.long_time(lc.LONG_FRAMES) < 2 ** 32
    assert set(lc.FRESNEL) == {(c, p) for c in (0.0, 1.0, 0.5, 2.0, -0.5) for p in (0.0, 0.5, 1.0, 5.0, 64.0, -1.0)}
    assert len(lc.FRESNEL_DROPPED) <= 1
    assert set(lc.SHAPES) == {(16, 4096), (4096, 16), (65535, 16), (31, 47), (17, 16)} and lc.NO_TILE_SHAPE == (15, 40)
    assert lc.TILED_SHAPES == tuple(lc.SHAPES)[:3] and set(lc.TILINGS) == {(0, 2), (1, 2), (0, 3), (2, 3), (0, 7), (6, 7)}
    for size, runs in lc.SHAPES.items():
        for scene in ("C2", "C3"):                       # both the one-frame and the primary-pass kernels, or one run
            frames = {f for s, f in runs if s == scene}
            assert frames == {1, 2} or (size == (65535, 16) and len(frames) == 1), (size, scene)
    assert set(rc.SCALAR_CASES) == set(lc.REF_CASES) and len(lc.REF_CASES) == 8


def test_scenes_reach_the_kernels_they_are_meant_for(native):
    """From the scenes' flags alone, through the restatement of build_params
    and launch_scene in tests/flag_lattice.py."""
    for scene in lc.SCENES:
        assert lc.kernel_of(scene) == lc.KERNEL[scene], scene
        has_mesh = lc.scene_of(scene).get("mesh_flat") is not None and not lc.scene_of(scene).get("example_sphere")
        assert (lc.LAUNCH_KIND[scene] == "path_pool") == has_mesh, scene
    assert {lc.KERNEL[s] for s in lc.SEED_SCENES} == {"spec_c1", "spec_c2", "spec_c3", "cls_cornell_mesh"}
    assert {lc.KERNEL[s] for s in lc.CAMERA_SCENES} == {"spec_c1", "spec_c2", "spec_c3", "spec_c4"}
    assert {lc.KERNEL[s] for s in lc.FRESNEL_SCENES} == {"spec_c3", "cls_cornell_mesh", "cls_cornell_sphere"}
    for scene in lc.FRESNEL_SCENES:                      # the scenes whose hits read the Fresnel pair: a specular map
        assert lc.scene_of(scene).get("tex_specular") is not None, scene


# ---- 1. time seeds -------------------------------------------------------------------------
@pytest.mark.parametrize("scene", lc.SEED_SCENES)
def test_seed_conditions_hold_on_the_oracle(oracle, native, scene):
    """A time of 2^24 and more must not render like the time a 24-bit
    multiply, a dropped sign or a dropped top bit would make of it."""
    hit = float(lc.hit_mask(scene).mean())
    assert hit == 1.0 if lc.scene_of(scene).get("cornell") else 0.15 < hit < 1.0, hit
    for t, narrow, _, least in lc.SEED_PAIRS:
        share = lc.seed_share(scene, t, narrow)
        print(f"{scene}: time {t:#x} against {narrow:#x}: {share:.4f} of the hit pixels in rows y >= 1 differ")
        assert share >= least, (scene, hex(t), share)
    # 2^31 against 0: y * 2^31 is 0 on the even rows, so only the odd rows may differ
    a, b = (lc.region(lc.oracle_render(scene, lc.frame_times(t))[0]) for t in (2 ** 31, 0))
    assert not lc.differing(a, b)[0::2].any()
    # every step of the walk is an image of its own, and none has a NaN
    steps = [lc.oracle_render(scene, ts)[0] for _, ts in lc.SEED_WALK + lc.SEED_WALK_TIME_SEED[:-1]]
    assert len({s.tobytes() for s in steps}) == len(steps)
    assert not any(np.isnan(s).any() for s in steps)


# ---- 2. long accumulations ---------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["C1", "C2"])
def test_long_expectation_is_what_the_oracle_accumulates(oracle, native, scene):
    """The per-pixel sum of vro_trace_sample results against vro_render over
    two calls of 64 frames; and the frames past 65,536 trace other paths than
    the frames a 16-bit frame number would make of them."""
    sc = lc.long_scene(scene)
    n = 2 * lc.LONG_CALL
    times = [lc.long_time(f) for f in range(1, n + 1)]
    a = po.render(sc, frames=lc.LONG_CALL, times=times[:lc.LONG_CALL], libm=po.LIBM_PORTABLE)[0]
    a = po.render(sc, frames=lc.LONG_CALL, times=times[lc.LONG_CALL:], first_frame=lc.LONG_CALL + 1,
                  libm=po.LIBM_PORTABLE, accum=a)[0]
    want = lc.long_expectation(scene, n)
    for (x, y), v in want.items():
        assert v.tobytes() == a[y, x].tobytes(), (scene, x, y, v, a[y, x])
    assert len({v.tobytes() for v in want.values()}) == len(want)
    # the camera is close: every sampled camera ray hits within 150 units (depth term below 1 per sample)
    assert all(0.0 < v[3] < 2 * n for v in want.values())
    L = po.lib()
    s = po.OracleScene(sc, libm=po.LIBM_PORTABLE)
    o = [np.zeros(4, np.float32), np.zeros(4, np.float32)]
    ptr = [v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for v in o]
    for x, y in lc.LONG_PIXELS:
        differ = 0
        for frame in range(65537, lc.LONG_FRAMES + 1):
            for k, f in enumerate((frame, frame & 0xFFFF)):
                L.vro_trace_sample(ctypes.byref(s.s), x, y, f, lc.long_time(frame), 0, ptr[k])
            differ += o[0].tobytes() != o[1].tobytes()
        print(f"{scene} pixel ({x}, {y}): {differ} of {lc.LONG_CALL} frames past 65,536 differ under a 16-bit frame number")
        # s1 = x * frame: column 0 cannot tell (row 0, where s2 = 0, is left open: the corners are there for the
        # tile's edges); elsewhere most frames must (a path that hits the light at once cannot)
        if x == 0:
            assert differ == 0, (scene, x, y, differ)
        elif y > 0:
            assert differ >= lc.LONG_CALL // 2, (scene, x, y, differ)
    assert sum(x > 0 and y > 0 for x, y in lc.LONG_PIXELS) >= 5


# ---- 3. camera ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.CAMERAS))
def test_camera_directions_are_finite_and_non_zero(oracle, native, name):
    """No case puts a NaN ray into traversal: the un-normalised direction of
    every pixel is finite and non-zero, and vro_primary_ray's normalised one
    is a unit vector."""
    cam = lc.camera_of(name)
    assert all(np.isfinite(np.asarray(v, np.float32)).all() for v in cam.values())
    raw, unit = lc.camera_directions(name)
    assert np.isfinite(raw).all() and (np.abs(raw).max(-1) > 0).all()
    length = np.sqrt((unit.astype(np.float64) ** 2).sum(-1))
    assert np.isfinite(unit).all() and np.abs(length - 1.0).max() < 1e-6, (length.min(), length.max())
    # the restatement is the oracle's: its normalised directions are parallel to vro_primary_ray's
    mine = raw.astype(np.float64) / np.sqrt((raw.astype(np.float64) ** 2).sum(-1, keepdims=True))
    assert np.abs(mine - unit).max() < 1e-6


def test_camera_case_set():
    for name, (fields, on, hits) in lc.CAMERAS.items():
        assert set(fields) <= {"origin", "dir", "up", "right", "fov_scale"} and set(on) <= set(lc.CAMERA_SCENES), name
        assert set(hits) <= set(on) & {"C3", "C4"} and set(hits.values()) <= {"none", "some", "all"}, name
    cams = {n: lc.camera_of(n) for n in lc.CAMERAS}
    dot = lambda a, b: float(np.dot(np.asarray(a, np.float64), np.asarray(b, np.float64)))          # noqa: E731
    handed = lambda c: dot(np.cross(c["dir"], c["up"]), c["right"])                                # noqa: E731
    assert dot(cams["skewed"]["right"], cams["skewed"]["dir"]) != 0
    assert handed(cams["left_handed"]) < 0 < handed(cams["rolled"]) and handed(cams["up"]) > 0 and handed(cams["down"]) > 0
    assert dot(cams["dir_x10"]["dir"], cams["dir_x10"]["dir"]) == 100.0
    assert {cams[n]["fov_scale"] for n in cams if n.startswith("fov_")} == {1e-3, 10.0, 1e3, 0.0, -0.9}
    assert cams["up"]["dir"] == (0.0, 1.0, 0.0) and cams["down"]["dir"] == (0.0, -1.0, 0.0)
    inside = lambda o, c, r: dot(np.subtract(o, c), np.subtract(o, c)) < r * r                     # noqa: E731
    assert inside(cams["in_example"]["origin"], (0, 0, 0), 10.0)                   # k_example of oracle/vro.c
    assert inside(cams["in_small"]["origin"], (25, 0, 15), 3.5)                    # k_spheres[1]
    assert cams["behind_wall"]["origin"][2] < -100.0 and cams["far"]["origin"][2] == 1e4
    for scene in ("C2", "C3"):
        assert len(lc.cameras_on(scene)) >= 14
    # every sparse extreme is claimed somewhere
    claimed = {(s, v) for _, (_, _, hits) in lc.CAMERAS.items() for s, v in hits.items()}
    assert claimed == {(s, v) for s in ("C3", "C4") for v in ("none", "some", "all")} - {("C3", "all")}


@pytest.mark.parametrize("scene", lc.CAMERA_SCENES)
def test_camera_conditions_hold_on_the_oracle(oracle, native, scene):
    base = lc.region(lc.oracle_render(scene)[0])
    for name in lc.cameras_on(scene):
        a = lc.oracle_render(scene, camera=name)[0]
        assert not np.isnan(a).any(), (scene, name)
        assert np.any(lc.region(a)[..., :3] != 0), f"{scene} {name}: a black image"
        change = float(lc.differing(lc.region(a), base).mean())
        hit = float(lc.hit_mask(scene, name).mean())
        print(f"{scene} {name}: {change:.4f} of the pixels differ from the default camera's; camera rays that hit {hit:.4f}")
        assert change >= lc.MIN_CAMERA_CHANGE, (scene, name, change)
        claim = lc.CAMERAS[name][2].get(scene)
        if claim is not None:
            assert {"none": hit == 0.0, "all": hit == 1.0, "some": 0.0 < hit < 1.0}[claim], (scene, name, claim, hit)


# ---- 4. Fresnel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", lc.FRESNEL_SCENES)
def test_fresnel_conditions_hold_on_the_oracle(oracle, native, scene):
    """At most 5 % of the pixels hold a NaN and at least 1 % differ from the
    (0.1, 3) image, for every pair that runs on the scene; a pair is dropped
    only for missing one of the two."""
    base = lc.region(lc.oracle_render(scene)[0])
    for pair in lc.FRESNEL:
        a = lc.oracle_render(scene, fresnel=pair)[0]
        nan = float(lc.nan_pixels(a).mean())
        change = float(lc.differing(lc.region(a), base).mean())
        print(f"{scene} {pair}: NaN share {nan:.4f}, {change:.4f} of the pixels differ from (0.1, 3)")
        ok = nan <= lc.MAX_NAN and change >= lc.MIN_FRESNEL_CHANGE
        assert ok == (pair in lc.fresnel_on(scene)), (scene, pair, nan, change)
        assert not np.isnan(lc.region(a)[..., 3]).any() and np.any(lc.region(a)[..., :3] != 0)


# ---- 5. image shapes ---------------------------------------------------------------------------------------
def test_shapes_are_what_the_names_say(native):
    assert lc.MAX_WIDTH == 65535 and (lc.MAX_WIDTH // 16) * 16 - 1 == 65519 < 2 ** 16       # x packed into 16 bits
    assert ((31 // 16) * 16, (47 // 16) * 16) == (16, 32) and ((17 // 16) * 16, 16) == (16, 16)
    w, h = lc.NO_TILE_SHAPE
    assert (w // 16) * (h // 16) == 0 and not lc.owned_mask(w, h, 0, 1).any()
    assert (16 // 16, 4096 // 16) == (1, 256) and (4096 // 16, 16 // 16) == (256, 1) and 65535 // 16 == 4095


@pytest.mark.parametrize("size", lc.TILED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_dealing_on_single_rows_and_columns(native, size):
    """vrhip_tile_pixels against the rule of include/vrhip.h, on the shapes
    where the row rotation degenerates: in a single column every row's
    rotation is a multiple of tiles_x, in a single row there is none."""
    w, h = size
    for n in (2, 3, 7):
        masks = [lc.owned_mask(w, h, r, n) for r in range(n)]
        total = np.zeros((h, w), np.int32)
        for r, m in enumerate(masks):
            mine = np.zeros((h, w), bool)
            for tx, ty in lc.dealt_tiles(w, h, r, n):
                mine[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = True
            assert np.array_equal(m, mine), (size, r, n)
            total += m
        covered = np.zeros((h, w), bool)
        covered[:(h // 16) * 16, :(w // 16) * 16] = True
        assert np.array_equal(total, covered.astype(np.int32))
        counts = [int(m.sum()) // 256 for m in masks]
        assert max(counts) - min(counts) <= 1 and min(counts) > 0, counts


@pytest.mark.parametrize("size", list(lc.SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_shape_images_vary_along_the_long_side(oracle, native, size):
    """A kernel that wrapped or clamped a coordinate would repeat part of the
    image.  On the oracle every tile that holds a pixel whose camera ray hits
    differs from every other such tile (every tile, in the Cornell box); the
    tiles of escaped rays alone may repeat, where neighbouring rays read the
    same HDRI texels."""
    w, h = size
    for scene, frames in lc.SHAPES[size]:
        a = lc.oracle_render(scene, lc.shape_times(frames), w=w, h=h)[0]
        assert not np.isnan(a).any() and np.any(lc.region(a)[..., :3] != 0), (size, scene, frames)
        assert not a[(h // 16) * 16:].any() and not a[:, (w // 16) * 16:].any()
        r = lc.region(a)
        ty, tx = r.shape[0] // 16, r.shape[1] // 16
        tiles = r.reshape(ty, 16, tx, 16, 4).transpose(0, 2, 1, 3, 4).reshape(ty * tx, -1)
        hit = lc.hit_mask(scene, None, w, h).reshape(ty, 16, tx, 16).transpose(0, 2, 1, 3).reshape(ty * tx, -1).any(-1)
        with_hit = [t.tobytes() for t in tiles[hit]]
        print(f"{w}x{h} {scene} {frames} frame(s): {len({t.tobytes() for t in tiles})} distinct tiles of {len(tiles)}, "
              f"{len(with_hit)} with a hit")
        assert len(with_hit) >= 1 and len(set(with_hit)) == len(with_hit), (size, scene, frames)
        if scene == "C2":
            assert hit.all()
