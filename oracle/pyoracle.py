"""ORACLE / TEST INFRASTRUCTURE ONLY -- ctypes binding of oracle/liboracle_vro.so.

Imported only by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
leg, as the checker.  The product (vrenderer_pathtracer_amd) never imports it.
The C restatement it binds follows /root/reference/cuda/src/PathTracer.cu
(see oracle/vro.c for per-function citations).
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "liboracle_vro.so")

LIBM_GLIBC = 0
LIBM_PORTABLE = 1

_f = ctypes.POINTER(ctypes.c_float)


class VroScene(ctypes.Structure):
    _fields_ = [
        ("cam_origin", ctypes.c_float * 4), ("cam_dir", ctypes.c_float * 4),
        ("cam_up", ctypes.c_float * 4), ("cam_right", ctypes.c_float * 4),
        ("fov_scale", ctypes.c_float),
        ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
        ("fresnel_coef", ctypes.c_float), ("fresnel_pow", ctypes.c_float),
        ("use_cornell", ctypes.c_int), ("use_example_sphere", ctypes.c_int),
        ("view_brdf", ctypes.c_int), ("mesh_initialised", ctypes.c_int),
        ("bvh", _f), ("n_bvh_f4", ctypes.c_size_t),
        ("verts", _f), ("normals", _f), ("tangents", _f), ("uvs", _f),
        ("n_slots", ctypes.c_size_t),
        ("hdr", _f), ("hdr_w", ctypes.c_uint32), ("hdr_h", ctypes.c_uint32),
        ("tex", _f * 3), ("tex_w", ctypes.c_uint32 * 3), ("tex_h", ctypes.c_uint32 * 3),
        ("brdf", _f),
        ("libm", ctypes.c_int), ("brute_force", ctypes.c_int),
    ]


COUNTER_FIELDS = ["paths", "rays", "node_visits", "slot_reads", "tri_tests", "hits",
                  "attr_bytes", "tex_fetches", "hdr_fetches", "brdf_fetches",
                  "pixel_io_bytes", "max_stack"]


class VroCounters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in COUNTER_FIELDS]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_FIELDS}


_lib = None


def build(force: bool = False) -> str:
    """Compile the oracle with its own Makefile (gcc, -ffp-contract=off)."""
    if force or not os.path.exists(_LIB_PATH):
        subprocess.run(["make", "-C", _HERE, "-s"], check=True)
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            build()
        L = ctypes.CDLL(_LIB_PATH)
        L.vro_render.restype = ctypes.c_int
        L.vro_render.argtypes = [ctypes.POINTER(VroScene), _f, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                 ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                 ctypes.POINTER(VroCounters)]
        L.vro_hash.restype = ctypes.c_uint32
        L.vro_hash.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.vro_rng_uniforms.argtypes = [ctypes.c_uint32, ctypes.c_int, _f]
        L.vro_intersect_triangle.argtypes = [_f] * 6
        L.vro_sphere_intersect.restype = ctypes.c_float
        L.vro_sphere_intersect.argtypes = [ctypes.c_int, _f, _f]
        L.vro_brdf_index.restype = ctypes.c_int
        L.vro_brdf_index.argtypes = [_f, _f, _f, _f, ctypes.c_int]
        L.vro_span.argtypes = [_f, _f]
        L.vro_primary_ray.argtypes = [ctypes.POINTER(VroScene), ctypes.c_uint32, ctypes.c_uint32, _f, _f]
        L.vro_trace_sample.argtypes = [ctypes.POINTER(VroScene), ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, _f]
        for n in ["vro_p_sinf", "vro_p_cosf", "vro_p_atanf", "vro_p_acosf"]:
            getattr(L, n).restype = ctypes.c_float
            getattr(L, n).argtypes = [ctypes.c_float]
        for n in ["vro_p_atan2f", "vro_p_powf"]:
            getattr(L, n).restype = ctypes.c_float
            getattr(L, n).argtypes = [ctypes.c_float, ctypes.c_float]
        _lib = L
    return _lib


def _fp(a):
    if a is None:
        return None
    return a.ctypes.data_as(_f)


class OracleScene:
    """Holds numpy arrays alive and a VroScene pointing at them."""

    def __init__(self, scene: dict, libm: int = LIBM_GLIBC, brute_force: bool = False):
        self._keep = []
        s = VroScene()
        cam = scene["camera"]
        for name in ("origin", "dir", "up", "right"):
            v = np.asarray(cam[name], dtype=np.float32)
            arr = getattr(s, "cam_" + name)
            for i in range(3):
                arr[i] = float(v[i])
            arr[3] = 0.0
        s.fov_scale = float(np.float32(cam["fov_scale"]))
        s.width, s.height = int(scene["width"]), int(scene["height"])
        s.fresnel_coef = float(np.float32(scene.get("fresnel_coef", 0.1)))
        s.fresnel_pow = float(np.float32(scene.get("fresnel_pow", 3.0)))
        s.use_cornell = int(bool(scene.get("cornell", False)))
        s.use_example_sphere = int(bool(scene.get("example_sphere", False)))
        s.view_brdf = int(bool(scene.get("view_brdf", False)))
        mesh = scene.get("mesh_flat")
        if mesh is not None:
            arrs = {k: np.ascontiguousarray(mesh[k], dtype=np.float32)
                    for k in ("bvh", "verts", "normals", "tangents", "uvs")}
            self._keep.append(arrs)
            s.bvh = _fp(arrs["bvh"]); s.n_bvh_f4 = arrs["bvh"].size // 4
            s.verts = _fp(arrs["verts"]); s.normals = _fp(arrs["normals"])
            s.tangents = _fp(arrs["tangents"]); s.uvs = _fp(arrs["uvs"])
            s.n_slots = arrs["verts"].size // 4
            s.mesh_initialised = 1
        hdr = scene.get("hdr")
        if hdr is not None:
            h = np.ascontiguousarray(hdr, dtype=np.float32)
            self._keep.append(h)
            s.hdr = _fp(h); s.hdr_h, s.hdr_w = h.shape[0], h.shape[1]
        for i, key in enumerate(("tex_diffuse", "tex_normal", "tex_specular")):
            t = scene.get(key)
            if t is not None:
                t = np.ascontiguousarray(t, dtype=np.float32)
                self._keep.append(t)
                s.tex[i] = _fp(t); s.tex_h[i], s.tex_w[i] = t.shape[0], t.shape[1]
        brdf = scene.get("brdf")
        if brdf is not None:
            b = np.ascontiguousarray(brdf, dtype=np.float32)
            assert b.size == 3 * 1458000
            self._keep.append(b)
            s.brdf = _fp(b)
        s.libm = libm
        s.brute_force = int(brute_force)
        self.s = s
        self.width, self.height = s.width, s.height


def render(scene: dict, frames: int = 1, times=None, first_frame: int = 1, libm: int = LIBM_GLIBC,
           rows=None, threads: int = 0, accum=None, count: bool = False, brute_force: bool = False):
    """Render frames first_frame..first_frame+frames-1 with the oracle.

    Returns (accum float32[H,W,4], rgba uint8[H,W,4], depth uint8[H,W,4], counters|None).
    """
    L = lib()
    os_ = OracleScene(scene, libm=libm, brute_force=brute_force)
    W, H = os_.width, os_.height
    if accum is None:
        accum = np.zeros((H, W, 4), dtype=np.float32)
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    depth = np.zeros((H, W, 4), dtype=np.uint8)
    if times is None:
        times = [scene.get("time", 12345)] * frames
    t = (ctypes.c_uint32 * frames)(*[int(v) & 0xFFFFFFFF for v in times])
    r0, r1 = (0, H) if rows is None else rows
    cnt = VroCounters() if count else None
    rc = L.vro_render(ctypes.byref(os_.s), _fp(accum), rgba.ctypes.data, depth.ctypes.data,
                      first_frame, frames, t, r0, r1, threads,
                      ctypes.byref(cnt) if cnt is not None else None)
    if rc != 0:
        raise RuntimeError(f"vro_render failed: {rc}")
    return accum, rgba, depth, (cnt.as_dict() if cnt is not None else None)


# ---- the reference itself, compiled for the host (oracle/ref/README.md) ----------
_REF_RECIPE = os.path.join(_HERE, "ref")
_REF_OUT = os.path.join(_HERE, "_ref")            # build products; never committed
_REF_CXX = os.environ.get("VRO_REF_CXX", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"))
_REF_FLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math"]
# the two sources with a construct a host compiler cannot parse: 5 asm statements, 1 launch
_REF_KERNEL_FILES = ["cuda/src/PathTracer.cu", "cuda/include/PathTracer.cuh", "cuda/include/RayIntersection.cuh",
                     "cuda/include/MathHelpers.cuh", "cuda/include/Utilities.cuh"]
REF_VARIANTS = ["glibc_zero", "glibc_pattern", "portable_zero", "portable_pattern", "portable_ubsan"]


def reference_path():
    """The reference checkout: $VRO_REFERENCE, else ../reference beside this repository."""
    p = os.environ.get("VRO_REFERENCE")
    if not p:
        p = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "reference")
    return p if os.path.isfile(os.path.join(p, "cuda", "src", "PathTracer.cu")) else None


def ref_compiler_versions() -> dict:
    first = lambda cmd: subprocess.run(cmd, capture_output=True, text=True).stdout.splitlines()[0].strip()
    return {"clang++": first([_REF_CXX, "--version"]), "python": first(["python3", "--version"])}


def build_reference(force: bool = False, variants=None):
    """Compile the reference's kernel source and its SBVH builder for the host
    into oracle/_ref/: ref_{glibc,portable}_{zero,pattern}, ref_portable_ubsan
    (-fsanitize=float-cast-overflow, a stand-alone program), sbvh_driver and
    rng_kat; with `variants`, only those kernel builds.  A target newer than
    the recipe and the reference's sources is kept.  Returns {name: path}, or
    None when no reference checkout exists or the recipe's compiler is missing."""
    ref = reference_path()
    if ref is None or not os.path.exists(_REF_CXX):
        return None
    import importlib.util
    spec = importlib.util.spec_from_file_location("vro_ref_rewrite", os.path.join(_REF_RECIPE, "rewrite.py"))
    rewrite = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rewrite)
    names = ["ref_" + v for v in (variants or REF_VARIANTS)] + ([] if variants else ["sbvh_driver", "rng_kat"])
    out = {n: os.path.join(_REF_OUT, n) for n in names}
    recipe = [os.path.join(_REF_RECIPE, f) for f in sorted(os.listdir(_REF_RECIPE))]
    recipe += [os.path.join(r, f) for r, _, fs in os.walk(os.path.join(_REF_RECIPE, "standin")) for f in fs]
    recipe += [os.path.join(ref, f) for f in _REF_KERNEL_FILES + ["src/SBVH.cpp", "src/BVHNodes.cpp", "include/SBVH.h"]]
    newest = max(os.path.getmtime(p) for p in recipe + [os.path.abspath(__file__), os.path.join(_HERE, "vro_math.c")])
    stale = [n for n, p in out.items() if force or not os.path.exists(p) or os.path.getmtime(p) < newest]
    if not stale:
        return out
    src = os.path.join(_REF_OUT, "src")
    rewrite.rewrite_tree([os.path.join(ref, f) for f in _REF_KERNEL_FILES], src, want_asm=5, want_launch=1)
    standin = os.path.join(_REF_RECIPE, "standin")
    run = lambda cmd: subprocess.run(cmd, check=True, capture_output=True, text=True)
    cc = _REF_CXX[:-2] if _REF_CXX.endswith("++") else _REF_CXX
    math_o = os.path.join(_REF_OUT, "vro_math.o")
    run([cc, "-std=gnu11", "-c"] + _REF_FLAGS + ["-I", _HERE, os.path.join(_HERE, "vro_math.c"), "-o", math_o])
    for n in stale:
        if not n.startswith("ref_"):
            continue
        libm, init = n[4:].split("_")
        flags = list(_REF_FLAGS)
        flags += ["-ftrivial-auto-var-init=" + ("pattern" if init == "pattern" else "zero")]
        if init == "ubsan":
            flags += ["-fsanitize=float-cast-overflow", "-g"]
        if libm == "portable":
            flags += ["-DVRO_REF_PORTABLE"]
        run([_REF_CXX, "-std=c++14", "-w"] + flags + ["-I", standin, "-I", _HERE, "-I", src, "-x", "c++",
             os.path.join(src, "PathTracer.cu"), os.path.join(_REF_RECIPE, "ref_driver.cpp"),
             os.path.join(_REF_RECIPE, "standin_impl.cpp"), "-x", "none", math_o, "-lm", "-o", out[n]])
    if "sbvh_driver" in stale:
        run([_REF_CXX, "-std=c++14", "-w"] + _REF_FLAGS + ["-I", standin, "-I", os.path.join(ref, "include"),
             os.path.join(ref, "src", "SBVH.cpp"), os.path.join(ref, "src", "BVHNodes.cpp"),
             os.path.join(_REF_RECIPE, "sbvh_driver.cpp"), "-o", out["sbvh_driver"]])
    if "rng_kat" in stale:
        build_rng_kat(_REF_CXX)
    return out


def build_rng_kat(cxx: str = "g++") -> str:
    """The known-answer program of the stand-in RNG (oracle/ref/rng_kat.cpp);
    needs no reference checkout."""
    os.makedirs(_REF_OUT, exist_ok=True)
    exe = os.path.join(_REF_OUT, "rng_kat")
    subprocess.run([cxx, "-std=c++14"] + _REF_FLAGS + ["-I", os.path.join(_REF_RECIPE, "standin"),
                    os.path.join(_REF_RECIPE, "rng_kat.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def write_ref_blob(path: str, scene: dict, times) -> None:
    """The scene file oracle/ref/ref_driver.cpp reads (layout: see its header)."""
    u32 = lambda *v: np.array(v, dtype=np.uint32).tobytes()
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).tobytes()
    cam = scene["camera"]
    with open(path, "wb") as f:
        f.write(u32(0x31425256, scene["width"], scene["height"], len(times), bool(scene.get("cornell", False)),
                    bool(scene.get("example_sphere", False)), bool(scene.get("view_brdf", False))))
        for k in ("origin", "dir", "up", "right"):
            f.write(f32(np.asarray(cam[k], dtype=np.float32)[:3]))
        f.write(f32([cam["fov_scale"], scene.get("fresnel_coef", 0.1), scene.get("fresnel_pow", 3.0)]))
        f.write(u32(*[int(t) & 0xFFFFFFFF for t in times]))
        mesh = scene.get("mesh_flat")
        if mesh is None:
            f.write(u32(0, 0))
        else:
            f.write(u32(np.asarray(mesh["bvh"]).size // 4, np.asarray(mesh["verts"]).size // 4))
            for k in ("bvh", "verts", "normals", "tangents", "uvs"):
                f.write(f32(mesh[k]))
        for key in ("hdr", "tex_diffuse", "tex_normal", "tex_specular"):
            a = scene.get(key)
            if a is None:
                f.write(u32(0, 0))
            else:
                f.write(u32(a.shape[1], a.shape[0]))
                f.write(f32(a))
        brdf = scene.get("brdf")
        f.write(u32(brdf is not None))
        if brdf is not None:
            f.write(f32(brdf))


def render_reference(exe: str, scene: dict, times, workdir: str):
    """Run one reference build on `scene`, frames 1..len(times).  Returns
    (accum, rgba, depth, stderr text)."""
    blob, out = os.path.join(workdir, "scene.blob"), os.path.join(workdir, "out.bin")
    write_ref_blob(blob, scene, times)
    r = subprocess.run([exe, blob, out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{os.path.basename(exe)} failed ({r.returncode}): {r.stderr[-2000:]}")
    W, H = int(scene["width"]), int(scene["height"])
    raw = open(out, "rb").read()
    n = W * H
    assert len(raw) == n * 24
    accum = np.frombuffer(raw, np.float32, 4 * n, 0).reshape(H, W, 4).copy()
    rgba = np.frombuffer(raw, np.uint8, 4 * n, 16 * n).reshape(H, W, 4).copy()
    depth = np.frombuffer(raw, np.uint8, 4 * n, 20 * n).reshape(H, W, 4).copy()
    return accum, rgba, depth, r.stderr
