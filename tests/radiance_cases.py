"""Rays, scenes and the yardstick shared by the radiance-query tests
(test_radiance_cpu.py, test_gpu_radiance.py; vrhip_trace_radiance).

The yardstick is the oracle's own trace.  With up = right = (0, 0, 0) in its
camera, cx and cy are zero vectors, so the camera ray of vro_trace_sample is
normalize(dir + 0 * sx + 0 * sy) = normalize(dir) from `origin`, whatever x
and y are: x and y then only seed the path (s1 = x * frame, s2 = y * time,
frame = time = 1).  The sum dir + (+-0) turns a -0 component into +0, so
every ray set here keeps its direction components non-zero.
test_radiance_cpu.py ties this to the reference-pinned renders: the camera
directions traced this way give pyoracle.render's first frame bit for bit.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import flag_lattice as fl
import pyoracle as po
import shading_cases as sh

# one combination per feature class, and a mixed one (flag_lattice.name_of)
COMBO_NAMES = ("cornell+mesh", "mesh+tex_d+tex_n+tex_s", "cornell+example", "example+view_brdf+brdf",
               "cornell+view_brdf+mesh+brdf+tex_d+tex_s")
K_MAX = 5                          # paths per ray the shared references hold
SAMPLES = (1, 2, 5)
MAX_DROPPED = 0.01                 # rays whose oracle record is not finite
# scenes of tests/shading_cases.py (odd-shaped maps, zero tangents, the example sphere with maps) and one whose NaNs
# are the point: there nothing is dropped, a channel is equal bit for bit or NaN in both, and w is never NaN
SHADING_NAMES = ("S_odd_C3", "D_tan0_C2N", "S_odd_C1T", "X_nrm0_tris_C3")
SHADING_SAMPLES = (1, 2)
TIME = fl.TIMES[0]


def combo_of(name):
    flags = name.split("+")
    assert all(f in fl.FLAGS for f in flags), name
    return tuple(int(f in flags) for f in fl.FLAGS)


COMBOS = tuple(combo_of(n) for n in COMBO_NAMES)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f2u8(f):
    """vr_math.hpp f2u8: truncate, saturate, NaN -> 0."""
    f = np.asarray(f, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(f != f, 0, np.clip(np.nan_to_num(f, nan=0.0), 0.0, 255.0)).astype(np.uint8)


def depth_byte(w):
    """What the depth image shows for a last path's w."""
    return f2u8((np.float32(1.0) - np.asarray(w, np.float32)) * np.float32(255.0))


# ---- rays ------------------------------------------------------------------------
def camera_dirs(scene) -> np.ndarray:
    """The un-normalised camera direction dir + cx * sx + cy * sy of every
    pixel, row-major [H * W, 3], in fp32 and in the operation order of
    build_params (vrhip_render.cpp) and camera_ray (vr_kernel.hpp)."""
    f32 = np.float32
    cam, W, H = scene["camera"], int(scene["width"]), int(scene["height"])
    fov = f32(cam["fov_scale"])
    d, up, right = (np.asarray(cam[k], f32) for k in ("dir", "up", "right"))
    cx = (fov * f32(W) / f32(H)) * right
    cy = fov * up
    sx = ((0.25 + np.arange(W, dtype=np.float64)) / float(W) - 0.5).astype(f32)
    sy = ((0.25 + np.arange(H, dtype=np.float64)) / float(H) - 0.5).astype(f32)
    out = (d[None, None, :] + cx[None, None, :] * sx[None, :, None]) + cy[None, None, :] * sy[:, None, None]
    assert out.dtype == f32
    return np.ascontiguousarray(out.reshape(-1, 3))


def camera_seeds(scene, time=TIME, frame=1) -> np.ndarray:
    """(x * frame, y * time) per pixel, row-major: the seeds render gives a pixel's first sample."""
    W, H = int(scene["width"]), int(scene["height"])
    x, y = np.meshgrid(np.arange(W, dtype=np.uint64), np.arange(H, dtype=np.uint64))
    s = np.stack([x * np.uint64(frame), y * np.uint64(time)], -1) & np.uint64(0xFFFFFFFF)
    return np.ascontiguousarray(s.reshape(-1, 2).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def ray_set(which):
    """(origins [n,3], dirs [n,3], seeds [n,2]), never written.
    A: the 1,024 camera rays of a 32 x 32 lattice scene, seeded as frame 1 at TIME.
    B: 512 rays from points uniform in [-40, 40]^3 around the knot, directions
       uniform on the sphere scaled by a length in [0.1, 10], seeds from a fixed generator."""
    if which == "A":
        sc = fl.scene_of(COMBOS[0])
        d = camera_dirs(sc)
        o = np.tile(np.asarray(sc["camera"]["origin"], np.float32), (len(d), 1))
        s = camera_seeds(sc)
    elif which == "B":
        rng = np.random.default_rng(20240521)
        n = 512
        o = rng.uniform(-40.0, 40.0, (n, 3)).astype(np.float32)
        v = rng.normal(0.0, 1.0, (n, 3))
        v /= np.sqrt((v * v).sum(-1, keepdims=True))
        d = (v * rng.uniform(0.1, 10.0, (n, 1))).astype(np.float32)
        s = rng.integers(0, 2**32, (n, 2), dtype=np.uint64).astype(np.uint32)
    else:
        raise ValueError(which)
    out = tuple(np.ascontiguousarray(a) for a in (o, d, s))
    assert (out[1] != 0).all(), "the yardstick's camera sum can turn a -0 into +0"
    for a in out:
        a.setflags(write=False)
    return out


# ---- the yardstick ------------------------------------------------------------------
def oracle_paths(scene, origins, dirs, seeds, k_max, libm=po.LIBM_PORTABLE) -> np.ndarray:
    """[n, k_max, 4]: path k of ray i, the k + 1'th trace on the seed stream
    (seeds[i, 0], seeds[i, 1]), by vro_trace_sample through a camera with
    up = right = 0."""
    L = po.lib()
    sc = dict(scene)
    sc["camera"] = dict(scene["camera"], up=(0.0, 0.0, 0.0), right=(0.0, 0.0, 0.0))
    osc = po.OracleScene(sc, libm=libm)
    o = np.ascontiguousarray(origins, np.float32)
    d = np.ascontiguousarray(dirs, np.float32)
    s = np.ascontiguousarray(seeds, np.uint32)
    out = np.zeros((len(o), k_max, 4), np.float32)
    buf = (ctypes.c_float * 4)()
    ref = ctypes.byref(osc.s)
    for i in range(len(o)):
        for a in range(3):
            osc.s.cam_origin[a] = float(o[i, a])
            osc.s.cam_dir[a] = float(d[i, a])
        for k in range(k_max):
            L.vro_trace_sample(ref, int(s[i, 0]), int(s[i, 1]), 1, 1, k, buf)
            out[i, k] = buf[:]
    return out


def record_of(paths, n_samples) -> np.ndarray:
    """The record of vrhip_trace_radiance from a ray's paths: rgb =
    ((0 + r_0 * c) + r_1 * c) + ... in fp32, w the last path's."""
    paths = np.asarray(paths, np.float32)
    c = np.float32(1.0) / np.float32(n_samples)
    io = np.zeros((len(paths), 3), np.float32)
    with np.errstate(all="ignore"):
        for k in range(n_samples):
            io = io + paths[:, k, :3] * c
    assert io.dtype == np.float32
    return np.ascontiguousarray(np.concatenate([io, paths[:, n_samples - 1, 3:4]], -1))


def oracle_radiance(scene, origins, dirs, seeds, n_samples, libm=po.LIBM_PORTABLE) -> np.ndarray:
    return record_of(oracle_paths(scene, origins, dirs, seeds, n_samples, libm), n_samples)


def kept(paths) -> np.ndarray:
    """The rays whose oracle paths are all finite; at most MAX_DROPPED may be dropped."""
    ok = np.isfinite(paths).all((1, 2))
    assert (~ok).sum() <= MAX_DROPPED * len(ok), f"{(~ok).sum()} of {len(ok)} rays have a non-finite oracle record"
    return ok


@functools.lru_cache(maxsize=None)
def reference(name, which, mesh="shallow"):
    """(paths [n, K_MAX, 4], kept [n]) of combination `name` on ray set
    `which`: computed once, shared by every test that needs it, never written."""
    po.build()
    o, d, s = ray_set(which)
    paths = oracle_paths(fl.scene_of(combo_of(name), mesh), o, d, s, K_MAX)
    ok = kept(paths)
    paths.setflags(write=False)
    ok.setflags(write=False)
    return paths, ok


@functools.lru_cache(maxsize=None)
def shading_reference(name, which):
    """(paths [n, 2, 4], kept [n]) of a shading case on ray set `which`; in a
    NaN case every ray is kept."""
    po.build()
    o, d, s = ray_set(which)
    paths = oracle_paths(sh.make_case(name), o, d, s, max(SHADING_SAMPLES))
    ok = np.ones(len(paths), bool) if name in sh.NAN_CASES else kept(paths)
    paths.setflags(write=False)
    ok.setflags(write=False)
    return paths, ok


def same_or_nan_in_both(got, want) -> np.ndarray:
    """Per record: every channel equal bit for bit, or NaN in both."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return ((u32(got) == u32(want)) | (np.isnan(got) & np.isnan(want))).all(-1)
