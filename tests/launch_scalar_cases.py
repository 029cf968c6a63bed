"""The scalars a launch carries by value (RenderParams): time seeds, frame
numbers, the camera, the Fresnel pair and the image shape.

One recipe per case, in the manner of shading_cases.py, shared by
tests/ref_cases.py (the `scalars` family of reference-rendered fixtures),
tests/test_launch_scalars_cpu.py (what each case pins, from the oracle alone)
and tests/test_gpu_launch_scalars.py (the HIP kernels against the portable-libm
oracle over launch kinds).  Unless a case says otherwise the image is 64 x 48,
two frames, the (24, 12) knot with leaves of 2.

  seeds     SEED_TIMES on C1, C2, C3 and C2D: s2 = y * time wraps in uint32
  long      a 16 x 16 image accumulated past frame 65,536: s1 = x * frame,
            1 / frame, and first_frame + f through launches and the service ring
  camera    CAMERAS: poses at the poles of the HDRI lookup, inside spheres,
            outside the box, far away, rolled; bases that are scaled, skewed,
            long or left-handed; fov_scale from 0 to 1e3 and negative
  fresnel   FRESNEL pairs on C3, C2N and C1T
  shapes    SHAPES: single tile columns and rows, the widest image the ABI
            takes, truncated sizes, a size with no whole tile

What a case pins is measured on the oracle, not assumed: the conditions are in
tests/test_launch_scalars_cpu.py, with the measured shares beside the
thresholds.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import flag_lattice as fl
import pyoracle as po
import shading_cases as sh

W, H = 64, 48
KNOT = (24, 12)
GOLDEN_RATIO = 0x9E3779B9

# ---- scenes --------------------------------------------------------------------------
SCENES = ("C1", "C2", "C3", "C4", "C2D", "C2N", "C1T")
KERNEL = {"C1": "spec_c1", "C2": "spec_c2", "C3": "spec_c3", "C4": "spec_c4", "C2D": "cls_cornell_mesh",
          "C2N": "cls_cornell_mesh", "C1T": "cls_cornell_sphere"}
# vrhip_last_launch_info of a launch of the scene outside a service session and a graph
LAUNCH_KIND = {s: ("path_pool" if s in ("C2", "C3", "C2D", "C2N") else "render_kernel") for s in SCENES}


@functools.lru_cache(maxsize=None)
def _base(scene, w, h) -> dict:
    from vrenderer_pathtracer_amd import scenes
    if scene in ("C1", "C2", "C3", "C4"):
        sc = scenes.make_scene(scene, w, h, knot=KNOT)
    else:
        from test_gpu_classes import class_scene
        sc = class_scene(scene, w, h)
        if sc.get("mesh_flat") is not None:
            sc["mesh_flat"] = scenes.knot_flat(*KNOT)
    return sc


def scene_of(scene, w=W, h=H, camera=None, fresnel=None) -> dict:
    """A fresh scene dict; camera: a name of CAMERAS; fresnel: (coef, pow)."""
    sc = dict(_base(scene, w, h))
    if camera is not None:
        sc["camera"] = camera_of(camera)
    if fresnel is not None:
        sc["fresnel_coef"], sc["fresnel_pow"] = (float(v) for v in fresnel)
    return sc


def kernel_of(scene, strict=False) -> str:
    return fl.kernel_of(sh.combo_of(_base(scene, W, H)), strict)


def region(a):
    return a[:(a.shape[0] // 16) * 16, :(a.shape[1] // 16) * 16]


def differing(a, b) -> np.ndarray:
    """Pixels of two images of one kind that differ in any channel's bits."""
    if a.dtype == np.float32:
        return (a.view(np.uint32) != b.view(np.uint32)).any(-1)
    return (a != b).any(-1)


def _frozen(out):
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_render(scene, times=(12345, 13354), camera=None, fresnel=None, w=W, h=H, first_frame=1):
    """(accum, rgba8, depth8) of the portable-libm oracle: rendered once, shared, never written."""
    po.build()
    sc = scene_of(scene, w, h, camera, fresnel)
    return _frozen(po.render(sc, frames=len(times), times=list(times), first_frame=first_frame,
                             libm=po.LIBM_PORTABLE)[:3])


DEFAULT_TIMES = (12345, 13354)                    # ref_cases.times_of: two frames


# ---- 1. time seeds ---------------------------------------------------------------------
SEED_TIMES = (0, 1, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 1, GOLDEN_RATIO)
SEED_SCENES = ("C1", "C2", "C3", "C2D")
SEED_ROUTES = {"C1": ("plain",), "C2D": ("plain",),
               "C2": ("multi_frame", "one_frame", "graph", "service", "tiled", "time_seed"),
               "C3": ("multi_frame", "one_frame", "graph", "service", "tiled", "time_seed")}
# (time compared, the time a narrowed multiply or field would turn it into, rows compared, least share of the
# compared pixels that must differ): 24 bits kept, the sign dropped, bit 31 dropped
SEED_PAIRS = ((2 ** 24 + 1, 1, "y>=1", 0.90), (2 ** 32 - 1, 1, "y>=1", 0.90), (2 ** 31, 0, "y>=1", 0.45))


def frame_times(t) -> tuple:
    """The two frames' times of the walk step for time t: t itself and a second
    value 1009 later (mod 2^32), so that times[f] is indexed by the frame."""
    return (t, (t + 1009) & 0xFFFFFFFF)


# the walk of one context: a step per time, and one call whose two frames carry the same time
SEED_WALK = tuple((f"t={t:#x}", frame_times(t)) for t in SEED_TIMES) + (("repeat", (GOLDEN_RATIO, GOLDEN_RATIO)),)
# times=NULL, time_seed=t: every frame of the call carries t
SEED_WALK_TIME_SEED = tuple((f"seed={t:#x}", (t, t)) for t in SEED_TIMES)


def hit_mask(scene, camera=None, w=W, h=H) -> np.ndarray:
    """Pixels whose camera ray hits something: in an HDRI scene an escaped
    camera ray returns the depth term 1 exactly and draws no random number, a
    hit its distance / 150; a frame adds both samples' depth terms unhalved
    (mul4s leaves w alone).  Every camera ray of a Cornell scene hits."""
    sc = scene_of(scene, w, h, camera)
    if sc.get("cornell"):
        return np.ones((h // 16 * 16, w // 16 * 16), bool)
    a = oracle_render(scene, (12345,), camera, None, w, h)[0]
    return region(a)[..., 3] != 2.0


def seed_share(scene, t, t_narrow) -> float:
    """Share of the pixels in rows y >= 1 whose camera ray hits on which the
    two-frame accumulations for frame_times(t) and frame_times(t_narrow) differ."""
    a = region(oracle_render(scene, frame_times(t))[0])
    b = region(oracle_render(scene, frame_times(t_narrow))[0])
    m = hit_mask(scene).copy()
    m[0] = False
    return float(differing(a, b)[m].mean())


# ---- 2. long accumulations -----------------------------------------------------------------
LONG_W = LONG_H = 16
LONG_CALL = 64                                    # frames per call: kMaxFramesPerLaunch
LONG_FRAMES = 65536 + LONG_CALL                   # 1,025 calls: frames 1 .. 65,600
LONG_TIME0 = 2 ** 24 - 4096                       # the times cross 2^24 on the way
# the example sphere (radius 10 at the origin) from 18 units; the knot's tube at (45, 0, 0) from 30 units
LONG_CAMERAS = {"C1": dict(origin=(0.0, 0.0, 18.0)), "C2": dict(origin=(45.0, 0.0, 30.0))}
LONG_PIXELS = ((0, 0), (15, 0), (0, 15), (15, 15), (7, 8), (8, 7), (3, 12), (12, 3))


def long_time(frame) -> int:
    """The time of frame `frame` (1-based)."""
    return (LONG_TIME0 + 7 * frame) & 0xFFFFFFFF


def long_scene(scene) -> dict:
    sc = scene_of(scene, LONG_W, LONG_H)
    sc["camera"] = dict(sc["camera"], **LONG_CAMERAS[scene])
    return sc


@functools.lru_cache(maxsize=None)
def long_expectation(scene, frames=LONG_FRAMES):
    """{(x, y): float32[4]}: the accumulation of LONG_PIXELS after `frames`
    frames, one vro_trace_sample call per frame and sample, added in fp32 in
    path order as render_row does: the colour x 0.5, the depth term as it is
    (mul4s scales x, y and z only)."""
    po.build()
    L = po.lib()
    s = po.OracleScene(long_scene(scene), libm=po.LIBM_PORTABLE)
    out4 = np.zeros(4, np.float32)
    ptr, ref = out4.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(s.s)
    half = np.float32(0.5)
    out = {}
    for x, y in LONG_PIXELS:
        acc = np.zeros(4, np.float32)
        for frame in range(1, frames + 1):
            t = long_time(frame)
            for sample in (0, 1):
                L.vro_trace_sample(ref, x, y, frame, t, sample, ptr)
                acc[:3] += out4[:3] * half
                acc[3] += out4[3]
        acc.setflags(write=False)
        out[(x, y)] = acc
    return out


# ---- 3. camera ---------------------------------------------------------------------------------
def _cam(**kw) -> dict:
    from vrenderer_pathtracer_amd import scenes
    return dict(scenes.default_camera(), **kw)


# name -> (camera fields that differ from the default pose, scenes it runs on, {scene: share of camera rays that
# hit: "none", "all" or "some"} for the HDRI scenes of the sparse extremes).  right = dir x up in the default pose.
CAMERAS = {
    # poses
    "up": (dict(origin=(0.0, -150.0, 0.0), dir=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0)), ("C3", "C4"), {"C3": "some", "C4": "some"}),
    "down": (dict(origin=(0.0, 150.0, 0.0), dir=(0.0, -1.0, 0.0), up=(0.0, 0.0, -1.0)), ("C3", "C4"), {"C3": "some", "C4": "some"}),
    "sky": (dict(dir=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0)), ("C3", "C4"), {"C3": "none", "C4": "none"}),
    "in_example": (dict(origin=(0.0, 0.0, 5.0)), ("C1", "C4"), {"C4": "all"}),
    "in_small": (dict(origin=(25.0, 0.0, 15.0)), ("C1", "C2"), {}),
    "behind_wall": (dict(origin=(0.0, 0.0, -120.0), dir=(0.0, 0.0, 1.0), right=(-1.0, 0.0, 0.0)), ("C1", "C2"), {}),
    "far": (dict(origin=(0.0, 0.0, 1e4)), ("C1", "C2", "C3", "C4"), {"C3": "none", "C4": "none"}),
    "rolled": (dict(up=(1.0, 0.0, 0.0), right=(0.0, -1.0, 0.0)), ("C1", "C2", "C3", "C4"), {}),
    # bases
    "basis_x3": (dict(up=(0.0, 3.0, 0.0), right=(3.0, 0.0, 0.0)), ("C1", "C2", "C3", "C4"), {"C3": "some", "C4": "some"}),
    "basis_third": (dict(up=(0.0, 1.0 / 3.0, 0.0), right=(1.0 / 3.0, 0.0, 0.0)), ("C1", "C2", "C3", "C4"),
                    {"C3": "some", "C4": "some"}),
    "skewed": (dict(right=(1.0, 0.0, -0.5)), ("C1", "C2", "C3", "C4"), {}),
    "dir_x10": (dict(dir=(0.0, 0.0, -10.0)), ("C1", "C2", "C3", "C4"), {"C3": "none", "C4": "all"}),
    "left_handed": (dict(right=(-1.0, 0.0, 0.0)), ("C1", "C2", "C3", "C4"), {}),
    # fov_scale
    "fov_1e-3": (dict(fov_scale=1e-3), ("C1", "C2", "C3", "C4"), {"C3": "none", "C4": "all"}),
    "fov_10": (dict(fov_scale=10.0), ("C1", "C2", "C3", "C4"), {"C3": "some", "C4": "none"}),
    "fov_1e3": (dict(fov_scale=1e3), ("C1", "C2", "C3", "C4"), {"C3": "none", "C4": "none"}),
    "fov_0": (dict(fov_scale=0.0), ("C1", "C2", "C3", "C4"), {"C3": "none", "C4": "all"}),
    "fov_neg": (dict(fov_scale=-0.9), ("C1", "C2", "C3", "C4"), {}),
}
CAMERA_SCENES = ("C1", "C2", "C3", "C4")
MIN_CAMERA_CHANGE = 0.01


def camera_of(name) -> dict:
    return _cam(**CAMERAS[name][0])


def cameras_on(scene) -> tuple:
    return tuple(n for n, (_, on, _) in CAMERAS.items() if scene in on)


def camera_directions(name, w=W, h=H):
    """(un-normalised, normalised) camera directions of every pixel: the first
    restated here in fp32 (camera_basis and primary_ray of oracle/vro.c), the
    second from vro_primary_ray."""
    cam = camera_of(name)
    f32 = np.float32
    fov = f32(cam["fov_scale"])
    cx = (fov * f32(w) / f32(h)) * np.asarray(cam["right"], f32)
    cy = fov * np.asarray(cam["up"], f32)
    sx = ((0.25 + np.arange(w, dtype=np.float64)) / w - 0.5).astype(f32)
    sy = ((0.25 + np.arange(h, dtype=np.float64)) / h - 0.5).astype(f32)
    raw = (np.asarray(cam["dir"], f32)[None, None] + cx[None, None] * sx[None, :, None]) + cy[None, None] * sy[:, None, None]
    po.build()
    L = po.lib()
    s = po.OracleScene(scene_of("C1", w, h, name), libm=po.LIBM_PORTABLE)
    o4, d4 = np.zeros(4, np.float32), np.zeros(4, np.float32)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))           # noqa: E731
    unit = np.zeros((h, w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            L.vro_primary_ray(ctypes.byref(s.s), x, y, fp(o4), fp(d4))
            unit[y, x] = d4[:3]
    return raw.astype(np.float32), unit


# ---- 4. Fresnel ------------------------------------------------------------------------------------
FRESNEL_COEFS = (0.0, 1.0, 0.5, 2.0, -0.5)
FRESNEL_POWS = (0.0, 0.5, 1.0, 5.0, 64.0, -1.0)
FRESNEL_SCENES = ("C3", "C2N", "C1T")
FRESNEL_DEFAULT = (0.1, 3.0)
MAX_NAN = 0.05
MIN_FRESNEL_CHANGE = 0.01
FRESNEL = tuple((c, p) for c in FRESNEL_COEFS for p in FRESNEL_POWS)
# (scene, pair) left out by what test_launch_scalars_cpu.py measures: on C1T, whose example sphere covers a ninth of
# the image, (-0.5, 1) changes 0.81 % of the pixels against (0.1, 3), under the 1 % a pair must change; it stays on
# C3 (4.8 %) and C2N (7.9 %).  No pair makes a NaN on any of the three scenes (1 - aoi is never negative there).
FRESNEL_DROPPED = {("C1T", (-0.5, 1.0))}


def fresnel_on(scene) -> tuple:
    return tuple(p for p in FRESNEL if (scene, p) not in FRESNEL_DROPPED)


def nan_pixels(accum) -> np.ndarray:
    return np.isnan(region(accum)).any(-1)


# ---- 5. image shapes -------------------------------------------------------------------------------------
# (width, height) -> [(scene, frames)].  The widest image renders 2 M oracle paths per frame: one run per scene, the
# one-frame kernels (x packed into 16 bits beside y) in the Cornell box, where every pixel's paths depend on x, the
# primary pass and the listed-pixel pass on C3
SHAPES = {
    (16, 4096): (("C2", 1), ("C2", 2), ("C3", 1), ("C3", 2)),
    (4096, 16): (("C2", 1), ("C2", 2), ("C3", 1), ("C3", 2)),
    (65535, 16): (("C2", 1), ("C3", 2)),
    (31, 47): (("C2", 1), ("C2", 2), ("C3", 1), ("C3", 2)),
    (17, 16): (("C2", 1), ("C2", 2), ("C3", 1), ("C3", 2)),
}
TILED_SHAPES = ((16, 4096), (4096, 16), (65535, 16))
TILINGS = tuple((r, n) for n in (2, 3, 7) for r in (0, n - 1))
NO_TILE_SHAPE = (15, 40)                          # no whole 16 x 16 tile: nothing is rendered
MAX_WIDTH = 65535                                 # vrhip_create: 1 .. 65535 pixels per side


def shape_times(frames) -> tuple:
    return DEFAULT_TIMES[:frames]


def owned_mask(w, h, rank, n_ranks) -> np.ndarray:
    """The pixels rank `rank` of n_ranks renders, from vrhip_tile_pixels."""
    from vrenderer_pathtracer_amd import tiles
    m = np.zeros(w * h, bool)
    m[tiles.owned_pixels(w, h, rank, n_ranks)] = True
    return m.reshape(h, w)


def dealt_tiles(w, h, rank, n_ranks) -> list:
    """(tile_x, tile_y) of the rank's tiles by the rule of include/vrhip.h
    (vrhip_set_tiling): positions rank, rank + n, ... of the dealing sequence,
    position s in row s / tiles_x, column (s % tiles_x + s / tiles_x) % tiles_x;
    row-major with one rank."""
    tiles_x, tiles_y = w // 16, h // 16
    out = []
    for s in range(rank, tiles_x * tiles_y, n_ranks):
        ty = s // tiles_x
        out.append(((s % tiles_x + ty) % tiles_x if n_ranks > 1 else s % tiles_x, ty))
    return out


# ---- 6. reference fixtures ---------------------------------------------------------------------------------
# name -> dict(scene, times, camera, fresnel, w, h): the cases of the `scalars` family of tests/ref_cases.py, each
# free of NaNs and of float-to-int conversions out of range but the depth byte's
REF_CASES = {
    "T_2p24p1_C2": dict(scene="C2", times=frame_times(2 ** 24 + 1)),
    "T_2p32m1_C2": dict(scene="C2", times=frame_times(2 ** 32 - 1)),
    "K_skewed_C3": dict(scene="C3", camera="skewed"),
    "K_fov_10_C3": dict(scene="C3", camera="fov_10"),
    "K_up_C3": dict(scene="C3", camera="up"),
    "F_0_0.5_C3": dict(scene="C3", fresnel=(0.0, 0.5)),
    "F_1_64_C3": dict(scene="C3", fresnel=(1.0, 64.0)),
    "I_16x64_C2": dict(scene="C2", w=16, h=64),
}


def ref_scene(name) -> dict:
    c = REF_CASES[name]
    sc = scene_of(c["scene"], c.get("w", W), c.get("h", H), c.get("camera"), c.get("fresnel"))
    sc["name"] = name
    return sc


def ref_times(name) -> list:
    return list(REF_CASES[name].get("times", DEFAULT_TIMES))
