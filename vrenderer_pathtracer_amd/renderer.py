"""Python host mirror of the reference's renderer interface, over the C ABI.

`VRendererHIP` has the method names, argument meanings and error behaviour of
the reference's abstract `vRenderer` (include/vRenderer.h:30-168) as
implemented by `vRendererCuda` (src/vRendererCuda.cpp), so tests read like
code driving the reference.  Differences, all deliberate:
  * errors raise VRHIPError instead of printing, writing errorlog.txt and
    calling exit(0) (src/vRendererCuda.cpp:454-467);
  * GL interop (registerTextureBuffer / registerDepthBuffer) is replaced by
    device RGBA8 buffers plus read-back (headless);
  * render(frames=K) renders K progressive frames in one device pass;
  * the RNG `_time` seed is explicit (the reference uses wall-clock ms,
    src/vRendererCuda.cpp:114,153).
"""
from __future__ import annotations

import ctypes
import time as _time

import numpy as np

from . import _native
from ._native import VRHIPError, check, fptr

BRDF_SAMPLING_RES_THETA_H = 90      # include/vRenderer.h:23-25
BRDF_SAMPLING_RES_THETA_D = 90
BRDF_SAMPLING_RES_PHI_D = 360
BRDF_TABLE_FLOATS = 3 * BRDF_SAMPLING_RES_THETA_H * BRDF_SAMPLING_RES_THETA_D * BRDF_SAMPLING_RES_PHI_D // 2

DIFFUSE, NORMAL, SPECULAR = 0, 1, 2     # vTextureType (cuda/include/PathTracer.cuh:86)


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


def build_flat(mesh: dict, max_leaf_tris: int = 2) -> dict:
    """Native BVH build + reference flattening (src/vRendererCuda.cpp:204-279).

    mesh: positions (N,3), normals (N,3), tangents (N,3), uvs (N,2), tris (M,3) uint32.
    Returns dict bvh (n,4), verts/normals/tangents (s,4), uvs (s,2) float32 arrays.
    """
    L = _native.lib()
    pos = _f32(mesh["positions"])
    nrm = _f32(mesh["normals"]) if mesh.get("normals") is not None else None
    tan = _f32(mesh["tangents"]) if mesh.get("tangents") is not None else None
    uvs = _f32(mesh["uvs"]) if mesh.get("uvs") is not None else None
    tris = np.ascontiguousarray(mesh["tris"], dtype=np.uint32)
    nv, nt = pos.shape[0], tris.shape[0]
    n_bvh = ctypes.c_size_t(0)
    n_slots = ctypes.c_size_t(0)
    tp = tris.ctypes.data_as(_native._u32)
    check(L.vrhip_build_flat(fptr(pos), fptr(nrm), fptr(tan), fptr(uvs), nv, tp, nt, max_leaf_tris,
                             None, ctypes.byref(n_bvh), None, None, None, None, ctypes.byref(n_slots)),
          "vrhip_build_flat(size)")
    out = {"bvh": np.zeros((n_bvh.value, 4), np.float32),
           "verts": np.zeros((n_slots.value, 4), np.float32),
           "normals": np.zeros((n_slots.value, 4), np.float32),
           "tangents": np.zeros((n_slots.value, 4), np.float32),
           "uvs": np.zeros((n_slots.value, 2), np.float32)}
    check(L.vrhip_build_flat(fptr(pos), fptr(nrm), fptr(tan), fptr(uvs), nv, tp, nt, max_leaf_tris,
                             fptr(out["bvh"]), ctypes.byref(n_bvh), fptr(out["verts"]), fptr(out["normals"]),
                             fptr(out["tangents"]), fptr(out["uvs"]), ctypes.byref(n_slots)),
          "vrhip_build_flat")
    return out


def validate_flat(flat: dict) -> tuple[int, int]:
    """Returns (depth, inner node count) of a flattened tree, raising if malformed."""
    L = _native.lib()
    d = ctypes.c_uint32(0)
    n = ctypes.c_uint32(0)
    bvh = _f32(flat["bvh"])
    verts = _f32(flat["verts"])
    check(L.vrhip_validate_flat(fptr(bvh), bvh.size // 4, fptr(verts), verts.size // 4, ctypes.byref(d),
                                ctypes.byref(n)), "vrhip_validate_flat")
    return d.value, n.value


def flat_sah_cost(flat: dict) -> float:
    """SAH cost of a flattened tree over its root's area, on the host
    (vrhip_flat_sah_cost): the definition VRendererHIP.bvh_sah_cost evaluates
    on the device.  Raises if the tree is malformed."""
    L = _native.lib()
    cost = ctypes.c_double(0.0)
    bvh = _f32(flat["bvh"])
    verts = _f32(flat["verts"])
    check(L.vrhip_flat_sah_cost(fptr(bvh), bvh.size // 4, fptr(verts), verts.size // 4, ctypes.byref(cost)),
          "vrhip_flat_sah_cost")
    return cost.value


RAY_MISS = 0xFFFFFFFF                    # VRHIP_RAY_MISS
RAYS_CLOSEST, RAYS_ANY = 0, 1           # vrhip_trace_rays modes
SURF_NONE, SURF_CORNELL, SURF_SMALL, SURF_EXAMPLE, SURF_MESH = range(5)   # vrhip_surface_hit kind (VRHIP_SURF_*)
# VRendererHIP.denoise defaults: the minimum of the CPU sweep recorded in profiles/denoise/README.md
DENOISE_SIGMA_COLOR, DENOISE_SIGMA_POSITION, DENOISE_NORMAL_POWER_LOG2 = 4.0, 32.0, 1


def _unpack_hits(rec, xp):
    """The (N,4) int32 records of vrhip_ray_hit as the dict the ray queries
    return: t, u, v float32 and prim int64 with -1 for a miss.  xp: numpy or torch."""
    prim = rec[:, 1].astype(np.int64) if xp is np else rec[:, 1].to(xp.int64)
    prim = xp.where(prim < 0, prim + (1 << 32), prim)          # the uint32 behind the int32
    prim = xp.where(prim == RAY_MISS, xp.full_like(prim, -1), prim)
    f = rec.view(np.float32) if xp is np else rec.view(xp.float32)
    if xp is np:
        return {"t": f[:, 0].copy(), "prim": prim, "u": f[:, 2].copy(), "v": f[:, 3].copy()}
    return {"t": f[:, 0].contiguous(), "prim": prim, "u": f[:, 2].contiguous(), "v": f[:, 3].contiguous()}


def flat_trace_rays(flat: dict, origins, dirs, tmax=None, any_hit: bool = False) -> dict:
    """Ray queries against a flattened tree on the host (vrhip_flat_trace_rays):
    one lane of the reference's walk, the yardstick of VRendererHIP.traceRays.
    origins, dirs (N,3) float32, tmax (N,) float32 or None (1e20).  Returns
    numpy arrays t, u, v (N,) float32 and prim (N,) int64: the slot of the hit
    triangle's first vertex in flat["verts"], -1 for a miss.  With any_hit
    only hit-or-miss is defined (a hit is t = 0, prim = 0).  Raises if the tree
    is malformed."""
    L = _native.lib()
    bvh = _f32(flat["bvh"])
    verts = _f32(flat["verts"])
    o = _f32(origins).reshape(-1, 3)
    d = _f32(dirs).reshape(-1, 3)
    n = o.shape[0]
    if d.shape[0] != n:
        raise ValueError(f"dirs: shape {d.shape} (expected ({n}, 3))")
    tm = None
    if tmax is not None:
        tm = _f32(tmax).reshape(-1)
        if tm.shape[0] != n:
            raise ValueError(f"tmax: shape {tm.shape} (expected ({n},))")
    rec = np.zeros((n, 4), np.int32)
    check(L.vrhip_flat_trace_rays(fptr(bvh), bvh.size // 4, fptr(verts), verts.size // 4, fptr(o), fptr(d), fptr(tm), n,
                                  RAYS_ANY if any_hit else RAYS_CLOSEST, ctypes.c_void_p(rec.ctypes.data)),
          "vrhip_flat_trace_rays")
    return _unpack_hits(rec, np)


_POWF_LUTS = {}


def texture_to_float4(rgba8: np.ndarray, gamma: float, tex_type: int) -> np.ndarray:
    """QImage pixels (uint8 (H,W,4), RGBA) -> the float4 texels
    vRendererCuda::loadTexture uploads (src/vRendererCuda.cpp:344-368):
    channel / 255.f; on DIFFUSE maps the colour channels raised to
    1.f / gamma with std::pow(float, float) -- libm's powf, applied here
    through a 256-entry table of its own results, so every texel rounds as
    the C++ host's does (numpy's float32 power may differ by an ulp)."""
    corr = np.float32(1.0) / np.float32(gamma) if gamma > 0.001 else np.float32(1.0)
    lin = np.arange(256, dtype=np.float32) / np.float32(255.0)
    if tex_type == DIFFUSE:
        key = float(corr)
        lut = _POWF_LUTS.get(key)
        if lut is None:
            libm = ctypes.CDLL("libm.so.6")
            libm.powf.restype = ctypes.c_float
            libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
            lut = np.array([libm.powf(float(v), key) for v in lin], np.float32)
            _POWF_LUTS[key] = lut
    else:
        lut = lin
    t = np.asarray(rgba8, np.uint8)
    return np.stack([lut[t[..., 0]], lut[t[..., 1]], lut[t[..., 2]], lin[t[..., 3]]], -1).astype(np.float32)


def load_merl(path: str) -> np.ndarray:
    """vBRDFLoader::loadBinary (src/BRDFLoader.cpp:15-50) through the C ABI:
    a MERL .binary file as float32[3*90*90*180] (planar R, G, B), ready for loadBRDF."""
    L = _native.lib()
    out = np.zeros(BRDF_TABLE_FLOATS, np.float32)
    check(L.vrhip_load_merl(str(path).encode(), fptr(out), out.size), "vrhip_load_merl")
    return out


def load_exr(path: str) -> np.ndarray:
    """The HDRI read of NGLScene::loadHDRMap (src/NGLScene.cpp:205-231,
    Imf::RgbaInputFile) through the C ABI: float16 (H, W, 4) RGBA over the data
    window, ready for VRendererHIP.loadHDR."""
    L = _native.lib()
    w = ctypes.c_uint32(0)
    h = ctypes.c_uint32(0)
    p = str(path).encode()
    check(L.vrhip_load_exr(p, None, 0, ctypes.byref(w), ctypes.byref(h)), "vrhip_load_exr")
    out = np.zeros((h.value, w.value, 4), np.uint16)
    check(L.vrhip_load_exr(p, out.ctypes.data_as(_native._u16), out.size, ctypes.byref(w), ctypes.byref(h)),
          "vrhip_load_exr")
    return out.view(np.float16)


class Camera:
    """Host camera state, the reference's Camera (src/Camera.cpp) reduced to
    what the renderer consumes: origin, dir, up, right, fovScale."""

    def __init__(self, origin=(0.0, 0.0, 150.0), dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0),
                 right=(1.0, 0.0, 0.0), fov_scale=None):
        self.origin = np.asarray(origin, np.float32)
        self.dir = np.asarray(dir, np.float32)
        self.up = np.asarray(up, np.float32)
        self.right = np.asarray(right, np.float32)
        self.fov_scale = np.float32(default_fov_scale() if fov_scale is None else fov_scale)
        self.dirty = False

    def is_dirty(self) -> bool:
        return self.dirty


def default_fov_scale() -> float:
    """Camera::getFovScale for the default 75 degree FOV (src/Camera.cpp:4,119-123), in fp32 + tanf."""
    libm = ctypes.CDLL("libm.so.6")
    libm.tanf.restype = ctypes.c_float
    libm.tanf.argtypes = [ctypes.c_float]
    k_deg_in_rad = np.float32(np.pi / np.float64(np.float32(180.0)))
    fov_rad = np.float32(np.float32(75.0) * k_deg_in_rad)
    return float(libm.tanf(float(np.float32(fov_rad / np.float32(2.0)))))


class VRendererHIP:
    """MI355X peer of vRendererCuda behind the vRenderer interface."""

    def __init__(self, device=0):
        """device: a GPU index, or a sequence of them for one renderer over
        several GPUs of this process (vrhip_create_multi: the tiles are dealt
        over the devices, the images gathered to the first)."""
        self._lib = _native.lib()
        self._ctx = ctypes.c_void_p(None)
        self._device = device
        self._camera = None
        self.m_fresnelCoef = 0.1     # src/vRendererCuda.cpp:27-28
        self.m_fresnelPow = 3.0
        self.width = self.height = 0
        self.default_time = None

    # -- vRenderer pure virtuals (include/vRenderer.h:48-133) ------------
    def init(self, w: int, h: int) -> None:
        assert w != 0 and h != 0
        if self._ctx:
            self.cleanUp()
        if isinstance(self._device, (list, tuple)):
            devs = (ctypes.c_int * len(self._device))(*[int(d) for d in self._device])
            check(self._lib.vrhip_create_multi(devs, len(self._device), w, h, ctypes.byref(self._ctx)),
                  "vrhip_create_multi")
        else:
            check(self._lib.vrhip_create(self._device, w, h, ctypes.byref(self._ctx)), "vrhip_create")
        self.width, self.height = w, h
        check(self._lib.vrhip_set_fresnel(self._ctx, self.m_fresnelCoef, self.m_fresnelPow), "vrhip_set_fresnel")

    def registerTextureBuffer(self, texture=None) -> None:
        """GL interop is replaced by the device RGBA8 buffer (read with read_rgba8)."""

    def registerDepthBuffer(self, depth_texture=None) -> None:
        """GL interop is replaced by the device depth buffer (read with read_depth8)."""

    def render(self, frames: int = 1, times=None, time_seed=None, sync: bool = True) -> None:
        self._need_ctx()
        if self._camera is not None and self._camera.is_dirty():
            self.updateCamera()
        arr = None
        if times is not None:
            arr = (ctypes.c_uint32 * frames)(*[int(t) & 0xFFFFFFFF for t in times])
        if time_seed is None:
            time_seed = self.default_time if self.default_time is not None else int(_time.time() * 1000)
        check(self._lib.vrhip_render(self._ctx, frames, arr, int(time_seed) & 0xFFFFFFFF), "vrhip_render")
        if sync:
            check(self._lib.vrhip_sync(self._ctx), "vrhip_sync")

    def cleanUp(self) -> None:
        if self._ctx:
            self._lib.vrhip_destroy(self._ctx)
            self._ctx = ctypes.c_void_p(None)

    def updateCamera(self) -> None:
        self._need_ctx()
        cam = self._camera or Camera()
        check(self._lib.vrhip_set_camera(self._ctx, fptr(_f32(cam.origin)), fptr(_f32(cam.dir)),
                                         fptr(_f32(cam.up)), fptr(_f32(cam.right)), float(cam.fov_scale)),
              "vrhip_set_camera")
        cam.dirty = False

    def initMesh(self, mesh: dict) -> None:
        """mesh: either a flattened dict (bvh/verts/normals/tangents/uvs, the
        layout vRendererCuda::initMesh produces) or an indexed triangle mesh
        (positions/normals/tangents/uvs/tris) that is built here."""
        self._need_ctx()
        flat = mesh if "bvh" in mesh else build_flat(mesh)
        arrs = {k: _f32(flat[k]) for k in ("bvh", "verts", "normals", "tangents", "uvs")}
        check(self._lib.vrhip_upload_mesh_flat(self._ctx, fptr(arrs["bvh"]), arrs["bvh"].size // 4,
                                               fptr(arrs["verts"]), fptr(arrs["normals"]),
                                               fptr(arrs["tangents"]), fptr(arrs["uvs"]),
                                               arrs["verts"].size // 4), "vrhip_upload_mesh_flat")

    DEVICE_BUILDERS = {"morton": 0, "sah": 1}          # vrhip_device_builder

    def initMeshDevice(self, positions, tris, normals=None, tangents=None, uvs=None, max_leaf_tris: int = 2,
                       builder="morton") -> None:
        """Build the mesh BVH on the GPU from torch tensors that live on the
        renderer's device (vrhip_upload_mesh_device_ex): positions, normals,
        tangents (N,3) float32, uvs (N,2) float32, tris (M,3) int32 or uint32,
        all contiguous; the optional arrays default to zeros.  builder:
        "morton" (the cheapest build) or "sah" (the tree build_flat makes on
        the host, built on the device: dearer to build, faster to render).
        ValueError for a wrong device, dtype or layout, or an unknown builder
        name (an integer is passed to the library as it is).  Synchronises
        torch's current stream on that device first (the build runs on the
        renderer's own stream)."""
        import torch
        self._need_ctx()
        if isinstance(builder, str):
            if builder not in self.DEVICE_BUILDERS:
                raise ValueError(f"builder: {builder!r} (expected 'morton' or 'sah')")
            builder = self.DEVICE_BUILDERS[builder]
        dev = self._torch_device()
        int_types = tuple(t for t in (torch.int32, getattr(torch, "uint32", None)) if t is not None)
        ptr = self._tensor_ptr
        p_pos = ptr("positions", positions, 3, (torch.float32,))
        p_tri = ptr("tris", tris, 3, int_types)
        if p_pos is None or p_tri is None:
            raise ValueError("positions and tris are required")
        nv, nt = int(positions.shape[0]), int(tris.shape[0])
        p_nrm = ptr("normals", normals, 3, (torch.float32,), nv)
        p_tan = ptr("tangents", tangents, 3, (torch.float32,), nv)
        p_uvs = ptr("uvs", uvs, 2, (torch.float32,), nv)
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_upload_mesh_device_ex(self._ctx, p_pos, p_nrm, p_tan, p_uvs, nv, p_tri, nt,
                                                    int(max_leaf_tris), int(builder)), "vrhip_upload_mesh_device")

    def refitMeshDevice(self, positions, normals=None, tangents=None) -> None:
        """Move the vertices of a mesh that initMeshDevice built, keeping its
        tree (vrhip_refit_mesh_device): positions (N,3) float32 for the N
        vertices of the upload; normals and tangents (N,3) float32 or None,
        and None KEEPS the resident ones (initMeshDevice's None means zeros).
        Tensors as for initMeshDevice (ValueError for a wrong device, dtype,
        shape or layout); the library's refusals raise VRHIPError and leave
        the mesh as it was.  Synchronises torch's current stream first.  The
        accumulation is not cleared (clearBuffer)."""
        import torch
        self._need_ctx()
        dev = self._torch_device()
        ptr = self._tensor_ptr
        p_pos = ptr("positions", positions, 3, (torch.float32,))
        if p_pos is None:
            raise ValueError("positions are required")
        nv = int(positions.shape[0])
        p_nrm = ptr("normals", normals, 3, (torch.float32,), nv)
        p_tan = ptr("tangents", tangents, 3, (torch.float32,), nv)
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_refit_mesh_device(self._ctx, p_pos, p_nrm, p_tan, nv), "vrhip_refit_mesh_device")

    def bvh_sah_cost(self) -> float:
        """SAH cost of the resident tree over its root's area (vrhip_bvh_sah_cost):
        what a refit tree is compared by against a rebuilt one."""
        cost = ctypes.c_double(0.0)
        check(self._lib.vrhip_bvh_sah_cost(self._need_ctx(), ctypes.byref(cost)), "vrhip_bvh_sah_cost")
        return cost.value

    def traceRays(self, origins, dirs, tmax=None, any_hit: bool = False) -> dict:
        """Where do these rays hit the resident mesh (vrhip_trace_rays)?
        origins, dirs: (N,3) float32 torch tensors on the renderer's GPU,
        contiguous; tmax: (N,) float32 or None (1e20).  Directions are used as
        given (t is in units of their length).  Only the triangle mesh is
        tested, whatever the scene flags say.  Returns device tensors t, u, v
        (N,) float32 and prim (N,) int64, -1 for a miss: the triangle's row in
        initMeshDevice's tris, or, for a mesh from initMesh, the slot of its
        first vertex in the flattened verts.  With any_hit only hit-or-miss is
        defined (a hit is t = 0, prim = 0).  ValueError for a wrong device,
        dtype, shape or layout.  Synchronises torch's current stream first;
        the query runs on the renderer's own stream and has finished on return."""
        import torch
        self._need_ctx()
        dev = self._torch_device()
        ptr = self._tensor_ptr
        p_o = ptr("origins", origins, 3, (torch.float32,))
        if p_o is None:
            raise ValueError("origins and dirs are required")
        n = int(origins.shape[0])
        p_d = ptr("dirs", dirs, 3, (torch.float32,), n)
        if p_d is None:
            raise ValueError("origins and dirs are required")
        p_t = ptr("tmax", tmax, None, (torch.float32,), n)
        rec = torch.empty((n, 4), dtype=torch.int32, device=f"cuda:{dev}")
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_trace_rays(self._ctx, p_o, p_d, p_t, n, RAYS_ANY if any_hit else RAYS_CLOSEST,
                                         ctypes.c_void_p(rec.data_ptr())), "vrhip_trace_rays")
        return _unpack_hits(rec, torch)

    def traceRadiance(self, origins, dirs, seeds=None, samples: int = 2):
        """What light arrives along these rays (vrhip_trace_radiance)?  The
        whole scene as render() would trace it now; the camera, the
        accumulation, the images and the frame counter play no part.
        origins, dirs: (N,3) float32 torch tensors on the renderer's GPU,
        contiguous; directions are normalised by the library.  seeds: (N,2)
        uint32 or int32, the seed pair each ray's first path starts from;
        None draws them with torch.randint on that device.  samples: paths
        per ray (1 to 4096), run one after the other on the ray's seed stream.
        Returns an (N,4) float32 device tensor: rgb the mean radiance of the
        paths, w the last path's depth term; a ray with a non-finite float or
        a direction of zero or overflowing length gives (0,0,0,0).
        ValueError for a wrong device, dtype, shape or layout.  Synchronises
        torch's current stream first; the query runs on the renderer's own
        stream and has finished on return."""
        import torch
        self._need_ctx()
        dev = self._torch_device()
        int_types = tuple(t for t in (torch.int32, getattr(torch, "uint32", None)) if t is not None)
        ptr = self._tensor_ptr
        p_o = ptr("origins", origins, 3, (torch.float32,))
        if p_o is None:
            raise ValueError("origins and dirs are required")
        n = int(origins.shape[0])
        p_d = ptr("dirs", dirs, 3, (torch.float32,), n)
        if p_d is None:
            raise ValueError("origins and dirs are required")
        if seeds is None:
            seeds = torch.randint(-2**31, 2**31, (n, 2), dtype=torch.int32, device=f"cuda:{dev}")
        p_s = ptr("seeds", seeds, 2, int_types, n)
        out = torch.empty((n, 4), dtype=torch.float32, device=f"cuda:{dev}")
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_trace_radiance(self._ctx, p_o, p_d, p_s, n, int(samples),
                                             ctypes.c_void_p(out.data_ptr())), "vrhip_trace_radiance")
        return out

    def traceSurface(self, origins, dirs) -> dict:
        """What does the path tracer see at the first hit of these rays
        (vrhip_trace_surface)?  The whole scene as render() would intersect it
        now: the Cornell box, the small spheres, the example sphere and the
        mesh, with the maps applied.  origins, dirs: (N,3) float32 torch
        tensors on the renderer's GPU, contiguous; directions are normalised
        by the library, so t is in world units.  Returns views of one (N,28)
        float32 device tensor (the dict's "record"): t (N,) float32; kind,
        prim, type (N,) int32 (kind: SURF_NONE .. SURF_MESH; prim: the sphere's
        index or the triangle as traceRays names it, -1 for a miss; type: 0
        specular, 1 diffuse, 2 BRDF); position, normal, tangent, color,
        specular, emission (N,3); bary and uv (N,2), a mesh hit's barycentrics
        and interpolated texture coordinates.  A miss has t = 1e20 and kind 0;
        a ray with a non-finite float or a direction of zero or overflowing
        length gives 28 zero words.  ValueError for a wrong device, dtype,
        shape or layout.  Synchronises torch's current stream first; the query
        runs on the renderer's own stream and has finished on return."""
        import torch
        self._need_ctx()
        dev = self._torch_device()
        ptr = self._tensor_ptr
        p_o = ptr("origins", origins, 3, (torch.float32,))
        if p_o is None:
            raise ValueError("origins and dirs are required")
        n = int(origins.shape[0])
        p_d = ptr("dirs", dirs, 3, (torch.float32,), n)
        if p_d is None:
            raise ValueError("origins and dirs are required")
        rec = torch.empty((n, 28), dtype=torch.float32, device=f"cuda:{dev}")
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_trace_surface(self._ctx, p_o, p_d, n, ctypes.c_void_p(rec.data_ptr())),
              "vrhip_trace_surface")
        return self._surface_dict(rec)

    @staticmethod
    def _surface_dict(rec) -> dict:
        """The views of an (N,28) float32 record tensor that traceSurface,
        surfaceAt and atlasRecords return."""
        import torch
        words = rec.view(torch.int32)
        return {"record": rec, "t": rec[:, 0], "kind": words[:, 1], "prim": words[:, 2], "type": words[:, 3],
                "position": rec[:, 4:7], "normal": rec[:, 8:11], "tangent": rec[:, 12:15], "color": rec[:, 16:19],
                "specular": rec[:, 20:23], "emission": rec[:, 24:27], "bary": rec[:, 7:12:4], "uv": rec[:, 19:24:4]}

    def surfaceAt(self, prims, bary) -> dict:
        """The surface records at points of the resident mesh, with no ray
        (vrhip_surface_at): what traceSurface would return for a hit of
        triangle prims[i] at barycentrics bary[i] = (u, v).  prims: (N,) int32,
        uint32 or int64 torch tensor on the renderer's GPU, the triangle as
        traceRays names it (the row of initMeshDevice's tris, or, for a mesh
        from initMesh, the slot of its first vertex in the flattened verts);
        int64 is narrowed here, a value outside 0 .. 2^32 - 2 naming no
        triangle.  bary: (N,2) float32, used as given (not clamped).  Returns
        traceSurface's dict with t = 0 and position the barycentric
        interpolation of the vertices; the maps and the BRDF view apply as
        render() would apply them now, the Cornell box and the example sphere
        play no part.  An entry whose prim names no triangle or whose u or v is
        not finite gives 28 zero words.  ValueError for a wrong device, dtype,
        shape or layout.  Synchronises torch's current stream first; the query
        runs on the renderer's own stream and has finished on return."""
        import torch
        self._need_ctx()
        dev = self._torch_device()
        int_types = tuple(t for t in (torch.int32, getattr(torch, "uint32", None)) if t is not None)
        if isinstance(prims, torch.Tensor) and prims.dtype == torch.int64:
            ok = (prims >= 0) & (prims < 0xFFFFFFFF)
            prims = torch.where(ok, prims, torch.full_like(prims, 0xFFFFFFFF)).to(torch.int32)
        p_p = self._tensor_ptr("prims", prims, None, int_types)
        if p_p is None:
            raise ValueError("prims and bary are required")
        n = int(prims.shape[0])
        p_b = self._tensor_ptr("bary", bary, 2, (torch.float32,), n)
        if p_b is None:
            raise ValueError("prims and bary are required")
        rec = torch.empty((n, 28), dtype=torch.float32, device=f"cuda:{dev}")
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_surface_at(self._ctx, p_p, p_b, n, ctypes.c_void_p(rec.data_ptr())), "vrhip_surface_at")
        return self._surface_dict(rec)

    def atlasRecords(self, width: int, height: int, gutter: int = 0) -> dict:
        """The surface records of a width x height lightmap atlas of the
        resident mesh's uvs (vrhip_atlas_surface; the definition:
        include/vrhip.h): texel (x, y), record y * width + x, holds the record
        of the point of the mesh whose uv is the texel's centre -- the texel
        render() fetches for that uv once the baked map is loaded with
        loadTexture.  Where several triangles cover a centre the smallest prim
        wins; an uncovered texel is a miss (kind 0, t = 1e20).  gutter (0 to
        64): dilation passes that give an uncovered texel the record of its
        first covered 8-neighbour, with t the pass that reached it; one pass is
        what a bake needs against black seams.  Returns traceSurface's dict,
        (width * height, 28); feed its "record" to shadeSurface and denoise.
        width, height 1 to 16384, at most 2^26 texels.  Synchronises torch's
        current stream first; the query runs on the renderer's own stream and
        has finished on return."""
        import torch
        self._need_ctx()
        dev = self._torch_device()
        vals = (width, height, gutter)
        if any(int(v) != v or not 0 <= int(v) < 2**32 for v in vals):
            raise ValueError("width, height and gutter are non-negative integers")
        w, h = int(width), int(height)
        n = w * h if w <= 16384 and h <= 16384 and w * h <= 2**26 else 1     # the library refuses the size
        rec = torch.empty((max(n, 1), 28), dtype=torch.float32, device=f"cuda:{dev}")
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_atlas_surface(self._ctx, w, h, int(gutter), ctypes.c_void_p(rec.data_ptr())),
              "vrhip_atlas_surface")
        return self._surface_dict(rec)

    def shadeSurface(self, hits, dirs, seeds=None, samples: int = 2):
        """What would the renderer show for these surfaces, seen along these
        directions (vrhip_shade_surface)?  The reference's trace with bounce
        0's hit given by the caller and bounces 1 to 3 traced through the
        whole scene as render() would trace it now.  hits: the (N,28) float32
        record tensor on the renderer's GPU, contiguous, or the dict
        traceSurface returns (its "record"); read are kind (0 a miss, 1 to 4 a
        hit), position, normal (used as given, not normalised), tangent, color,
        specular, emission and type.  dirs: (N,3) float32, the incoming
        direction of each record, normalised by the library.  seeds and
        samples as traceRadiance.  Returns an (N,4) float32 device tensor: rgb
        the mean radiance of the paths, w 0; a record whose direction has a
        non-finite float or zero or overflowing length, whose kind is above 4
        or which is a hit of a type above 2 gives (0,0,0,0).
        shadeSurface(traceSurface(o, d), d, s, k)[:, :3] is
        traceRadiance(o, d, s, k)[:, :3] bit for bit.  ValueError for a wrong
        device, dtype, shape or layout.  Synchronises torch's current stream
        first; the query runs on the renderer's own stream and has finished
        on return."""
        import torch
        self._need_ctx()
        dev = self._torch_device()
        int_types = tuple(t for t in (torch.int32, getattr(torch, "uint32", None)) if t is not None)
        ptr = self._tensor_ptr
        if isinstance(hits, dict):
            hits = hits.get("record")
        p_h = ptr("hits", hits, 28, (torch.float32,))
        if p_h is None:
            raise ValueError("hits and dirs are required")
        n = int(hits.shape[0])
        p_d = ptr("dirs", dirs, 3, (torch.float32,), n)
        if p_d is None:
            raise ValueError("hits and dirs are required")
        if seeds is None:
            seeds = torch.randint(-2**31, 2**31, (n, 2), dtype=torch.int32, device=f"cuda:{dev}")
        p_s = ptr("seeds", seeds, 2, int_types, n)
        out = torch.empty((n, 4), dtype=torch.float32, device=f"cuda:{dev}")
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_shade_surface(self._ctx, p_h, p_d, p_s, n, int(samples),
                                            ctypes.c_void_p(out.data_ptr())), "vrhip_shade_surface")
        return out

    def probeSH(self, points, dirs, weights=None, probe_seeds=None, dir_seeds=None, samples: int = 2):
        """What light arrives at these points, as nine spherical-harmonic
        coefficients per colour channel (vrhip_probe_sh)?  Ray (i, k) is the
        ray traceRadiance would trace from points[i] along dirs[k] with the
        seed pair probe_seeds[i] ^ dir_seeds[k]; its radiance is projected on
        the real SH basis to band 2 and summed over k in a fixed order inside
        the call, so no (N * K) buffer exists.  points: (N,3) float32 torch
        tensor on the renderer's GPU, contiguous.  dirs: (K,3) float32, one
        set shared by all probes (1 to 65536; scenes.probe_directions),
        normalised by the library.  weights: (K,) float32 quadrature weights,
        used as given; None weighs every direction 4 pi / K.  probe_seeds:
        (N,2), dir_seeds: (K,2) uint32 or int32; None draws them with
        torch.randint on that device.  samples: paths per ray (1 to 4096).
        Returns an (N,28) float32 device tensor: out[:, :27].view(N, 9, 3) is
        coefficient j of channel c, out[:, 27].view(torch.int32) the number of
        valid rays of the probe (a non-finite point or a direction of zero,
        non-finite or overflowing length contributes +0).  ValueError for a
        wrong device, dtype, shape or layout.  Synchronises torch's current
        stream first; the query runs on the renderer's own stream and has
        finished on return."""
        import torch
        self._need_ctx()
        dev = self._torch_device()
        int_types = tuple(t for t in (torch.int32, getattr(torch, "uint32", None)) if t is not None)
        ptr = self._tensor_ptr
        p_p = ptr("points", points, 3, (torch.float32,))
        p_d = ptr("dirs", dirs, 3, (torch.float32,))
        if p_p is None or p_d is None:
            raise ValueError("points and dirs are required")
        n, k = int(points.shape[0]), int(dirs.shape[0])
        p_w = ptr("weights", weights, None, (torch.float32,), k)
        if probe_seeds is None:
            probe_seeds = torch.randint(-2**31, 2**31, (n, 2), dtype=torch.int32, device=f"cuda:{dev}")
        if dir_seeds is None:
            dir_seeds = torch.randint(-2**31, 2**31, (k, 2), dtype=torch.int32, device=f"cuda:{dev}")
        p_ps = ptr("probe_seeds", probe_seeds, 2, int_types, n)
        p_ds = ptr("dir_seeds", dir_seeds, 2, int_types, k)
        out = torch.empty((n, 28), dtype=torch.float32, device=f"cuda:{dev}")
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_probe_sh(self._ctx, p_p, p_d, p_w, p_ps, p_ds, n, k, int(samples),
                                       ctypes.c_void_p(out.data_ptr())), "vrhip_probe_sh")
        return out

    def shIrradiance(self, sh, normals, index=None):
        """The irradiance the records of probeSH give at these normals
        (vrhip_sh_irradiance): the nine coefficients of each channel against
        the clamped-cosine lobe (pi, 2 pi / 3, pi / 4).  sh: (M,28) float32 on
        the renderer's GPU, contiguous.  normals: (N,3) float32, used as given
        (not normalised).  index: (N,) uint32 or int32, the record of each
        output; None takes record q for output q (then N == M).  Returns an
        (N,4) float32 device tensor (E.r, E.g, E.b, 0); an index of M or more
        gives zeros.  Needs no scene.  ValueError for a wrong device, dtype,
        shape or layout."""
        import torch
        self._need_ctx()
        dev = self._torch_device()
        int_types = tuple(t for t in (torch.int32, getattr(torch, "uint32", None)) if t is not None)
        ptr = self._tensor_ptr
        p_s = ptr("sh", sh, 28, (torch.float32,))
        p_n = ptr("normals", normals, 3, (torch.float32,))
        if p_s is None or p_n is None:
            raise ValueError("sh and normals are required")
        m, n = int(sh.shape[0]), int(normals.shape[0])
        p_i = ptr("index", index, None, int_types, n)
        if index is None and n != m:
            raise ValueError(f"normals: shape {tuple(normals.shape)} (expected ({m}, 3) without an index)")
        out = torch.empty((n, 4), dtype=torch.float32, device=f"cuda:{dev}")
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_sh_irradiance(self._ctx, p_s, m, p_i, p_n, n, ctypes.c_void_p(out.data_ptr())),
              "vrhip_sh_irradiance")
        return out

    def diffuseRecords(self, points, normals, color=None):
        """The (N,28) records of a white (or `color`ed) diffuse surface at
        these points and normals, for shadeSurface: what a lightmap texel or
        an irradiance probe stores.  kind SURF_MESH, prim -1, type 1 (diffuse),
        specular and emission 0, every other word 0.  points, normals: (N,3)
        float32 torch tensors on the renderer's GPU; color: (N,3), (3,) or
        None for (1,1,1).  The normals are normalised here, in torch: the
        library uses a record's normal as given.  Such a record does not depend
        on the direction passed with it; any valid one will do, for instance
        -normals.  The result carries the reference's own weight 2 * cos on a
        cosine-distributed sample and is not an irradiance in W/m^2 (a uniform
        incoming radiance L gives 4/3 L).  Built in torch only."""
        import torch
        dev = self._torch_device()
        ptr = self._tensor_ptr
        if ptr("points", points, 3, (torch.float32,)) is None:
            raise ValueError("points and normals are required")
        n = int(points.shape[0])
        if ptr("normals", normals, 3, (torch.float32,), n) is None:
            raise ValueError("points and normals are required")
        rec = torch.zeros((n, 28), dtype=torch.float32, device=f"cuda:{dev}")
        words = rec.view(torch.int32)
        words[:, 1] = SURF_MESH
        words[:, 2] = -1
        words[:, 3] = 1
        rec[:, 4:7] = points
        rec[:, 8:11] = normals / normals.norm(dim=1, keepdim=True)
        if color is None:
            rec[:, 16:19] = 1.0
        else:
            if not isinstance(color, torch.Tensor):
                color = torch.tensor(color, dtype=torch.float32, device=f"cuda:{dev}")
            if color.dtype != torch.float32 or color.device != rec.device or tuple(color.shape) not in ((3,), (n, 3)):
                raise ValueError("color: expected (3,) or (N,3) float32 on the renderer's GPU")
            rec[:, 16:19] = color
        return rec

    def cameraRays(self):
        """The current camera's rays (vrhip_camera_rays): (origins, dirs), each
        an (H*W, 3) float32 device tensor, pixel (x, y) in row y * W + x.  The
        directions are un-normalised, the operand of the camera ray's
        normalisation: traceSurface and traceRadiance normalise them as the
        render kernels do and so trace each pixel's own camera ray."""
        import torch
        self._need_ctx()
        if self._camera is not None and self._camera.is_dirty():
            self.updateCamera()
        dev = self._torch_device()
        n = int(self.width) * int(self.height)
        o = torch.empty((n, 3), dtype=torch.float32, device=f"cuda:{dev}")
        d = torch.empty((n, 3), dtype=torch.float32, device=f"cuda:{dev}")
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_camera_rays(self._ctx, ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(d.data_ptr())),
              "vrhip_camera_rays")
        return o, d

    # the defaults of denoise / denoiseFrame: chosen by the sweep in profiles/denoise/README.md
    DENOISE_DEFAULTS = dict(passes=5, sigma_color=DENOISE_SIGMA_COLOR, sigma_position=DENOISE_SIGMA_POSITION,
                            normal_power_log2=DENOISE_NORMAL_POWER_LOG2)

    @staticmethod
    def _denoise_params(passes, sigma_color, sigma_position, normal_power_log2, demodulate):
        vals = (passes, normal_power_log2)
        if any(int(v) != v or not 0 <= int(v) < 2**32 for v in vals):
            raise ValueError("passes and normal_power_log2 are non-negative integers")
        return _native.DenoiseParams(int(passes), 1 if demodulate else 0, int(normal_power_log2), float(sigma_color),
                                     float(sigma_position))

    def denoise(self, color, guides, passes: int = 5, sigma_color: float = DENOISE_SIGMA_COLOR,
                sigma_position: float = DENOISE_SIGMA_POSITION, normal_power_log2: int = DENOISE_NORMAL_POWER_LOG2,
                demodulate: bool = True, out=None):
        """The edge-avoiding a-trous filter on the caller's own grid
        (vrhip_denoise; the definition: include/vrhip.h): a view, a lightmap
        atlas, a probe sheet.  color: (H,W,4) float32 torch tensor on the
        renderer's GPU, contiguous, the mean radiance in rgb (w is carried
        through).  guides: the (H*W,28) record tensor of traceSurface or
        diffuseRecords, or the dict traceSurface returns; read are kind (1 to
        4: a valid cell), position, normal and color (the albedo).  passes 0 to
        8 at strides 1, 2, 4, ...; sigma_color and sigma_position in the units
        of the radiance and of the positions; normal_power_log2 m: the normal
        weight is max(N_p . N_q, 0)^(2^m); demodulate: filter colour / albedo
        and multiply the albedo back.  The defaults are DENOISE_DEFAULTS.  Returns an
        (H,W,4) tensor; out=color filters in place.  ValueError for a wrong
        device, dtype, shape or layout.  Synchronises torch's current stream
        first; the filter runs on the renderer's own stream and has finished on
        return."""
        import torch
        self._need_ctx()
        dev = self._torch_device()
        if isinstance(guides, dict):
            guides = guides.get("record")
        if not isinstance(color, torch.Tensor) or color.dim() != 3 or color.shape[2] != 4:
            raise ValueError("color: expected an (H, W, 4) torch tensor")
        h, w = int(color.shape[0]), int(color.shape[1])
        if h == 0 or w == 0:
            raise ValueError("color: an empty grid")
        p_c = self._tensor_ptr("color", color.view(h * w, 4) if color.is_contiguous() else color, 4, (torch.float32,))
        p_g = self._tensor_ptr("guides", guides, 28, (torch.float32,), h * w)
        if p_g is None:
            raise ValueError("color and guides are required")
        if out is None:
            out = torch.empty((h, w, 4), dtype=torch.float32, device=f"cuda:{dev}")
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (h, w, 4):
            raise ValueError(f"out: expected an ({h}, {w}, 4) torch tensor")
        p_o = self._tensor_ptr("out", out.view(h * w, 4) if out.is_contiguous() else out, 4, (torch.float32,))
        prm = self._denoise_params(passes, sigma_color, sigma_position, normal_power_log2, demodulate)
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_denoise(self._ctx, p_c, p_g, w, h, ctypes.byref(prm), p_o), "vrhip_denoise")
        return out

    def denoiseFrame(self, passes: int = 5, sigma_color: float = DENOISE_SIGMA_COLOR,
                     sigma_position: float = DENOISE_SIGMA_POSITION, normal_power_log2: int = DENOISE_NORMAL_POWER_LOG2,
                     demodulate: bool = True, rgba8: bool = False):
        """The rendered frames so far, filtered (vrhip_denoise_frame): colour
        is the accumulation divided by the frame count as the tonemap divides
        it, guides are traceSurface on cameraRays, made inside the library.
        Parameters as denoise.  Returns the (H,W,4) float32 device tensor, and
        with rgba8=True the pair (float image, (H,W,4) uint8 image: the
        render's own tonemap of the filtered colour).  The accumulation, the
        renderer's images and the frame count stay as they are.  VRHIPError
        before the first render, on a tiled rank and on a multi-device
        renderer."""
        import torch
        self._need_ctx()
        if self._camera is not None and self._camera.is_dirty():
            self.updateCamera()
        dev = self._torch_device()
        prm = self._denoise_params(passes, sigma_color, sigma_position, normal_power_log2, demodulate)
        h, w = int(self.height), int(self.width)
        out = torch.empty((h, w, 4), dtype=torch.float32, device=f"cuda:{dev}")
        img = torch.empty((h, w, 4), dtype=torch.uint8, device=f"cuda:{dev}") if rgba8 else None
        torch.cuda.current_stream(dev).synchronize()
        check(self._lib.vrhip_denoise_frame(self._ctx, ctypes.byref(prm), ctypes.c_void_p(out.data_ptr()),
                                            ctypes.c_void_p(img.data_ptr()) if rgba8 else None), "vrhip_denoise_frame")
        return (out, img) if rgba8 else out

    def _torch_device(self) -> int:
        """The GPU index device tensors must live on (a group's first device)."""
        if isinstance(self._device, (list, tuple)):
            return int(self._device[0])
        return int(self._device)

    def _tensor_ptr(self, name, t, cols, dtypes, rows=None):
        """The device pointer of an (N, cols) torch tensor on the renderer's
        GPU (cols None: an (N,) tensor), or None for None; ValueError for
        anything else."""
        import torch
        dev = self._torch_device()
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a torch tensor")
        if t.device.type != "cuda" or t.device.index != dev:
            raise ValueError(f"{name}: tensor is on {t.device}, the renderer on GPU {dev}")
        if t.dtype not in dtypes:
            raise ValueError(f"{name}: dtype {t.dtype} (expected {' or '.join(str(d) for d in dtypes)})")
        if cols is None:
            if t.dim() != 1 or (rows is not None and t.shape[0] != rows):
                raise ValueError(f"{name}: shape {tuple(t.shape)} (expected ({'N' if rows is None else rows},))")
        elif t.dim() != 2 or t.shape[1] != cols or (rows is not None and t.shape[0] != rows):
            raise ValueError(f"{name}: shape {tuple(t.shape)} (expected ({'N' if rows is None else rows}, {cols}))")
        if not t.is_contiguous():
            raise ValueError(f"{name}: tensor is not contiguous")
        return ctypes.c_void_p(t.data_ptr())

    def export_mesh_flat(self) -> dict:
        """The resident mesh in the reference layout (vrhip_export_mesh_flat):
        the dict build_flat returns, whichever call uploaded the mesh."""
        n_bvh = ctypes.c_size_t(0)
        n_slots = ctypes.c_size_t(0)
        check(self._lib.vrhip_export_mesh_flat(self._need_ctx(), None, ctypes.byref(n_bvh), None, None, None, None,
                                               ctypes.byref(n_slots)), "vrhip_export_mesh_flat(size)")
        out = {"bvh": np.zeros((n_bvh.value, 4), np.float32),
               "verts": np.zeros((n_slots.value, 4), np.float32),
               "normals": np.zeros((n_slots.value, 4), np.float32),
               "tangents": np.zeros((n_slots.value, 4), np.float32),
               "uvs": np.zeros((n_slots.value, 2), np.float32)}
        check(self._lib.vrhip_export_mesh_flat(self._ctx, fptr(out["bvh"]), ctypes.byref(n_bvh), fptr(out["verts"]),
                                               fptr(out["normals"]), fptr(out["tangents"]), fptr(out["uvs"]),
                                               ctypes.byref(n_slots)), "vrhip_export_mesh_flat")
        return out

    def loadHDR(self, pixels, w: int = None, h: int = None) -> None:
        """pixels: float32 (H,W,4) or float16 (H,W,4) (Imf::Rgba layout)."""
        self._need_ctx()
        a = np.ascontiguousarray(pixels)
        h = a.shape[0] if h is None else h
        w = a.shape[1] if w is None else w
        if a.dtype == np.float16:
            check(self._lib.vrhip_upload_hdr_half(self._ctx, a.view(np.uint16).ctypes.data_as(_native._u16), w, h),
                  "vrhip_upload_hdr_half")
        else:
            a = _f32(a)
            check(self._lib.vrhip_upload_hdr(self._ctx, fptr(a), w, h), "vrhip_upload_hdr")

    def loadTexture(self, texture, gamma: float = 1.0, type: int = DIFFUSE) -> None:
        """texture: uint8 (H,W,4) image (QImage pixels) -> float4 as
        vRendererCuda::loadTexture does (inverse gamma on DIFFUSE only,
        src/vRendererCuda.cpp:344-368); or a float32 (H,W,4) array used as is."""
        self._need_ctx()
        t = np.asarray(texture)
        if t.dtype == np.uint8:
            t = texture_to_float4(t, gamma, type)
        t = _f32(t)
        check(self._lib.vrhip_upload_texture(self._ctx, int(type), fptr(t), t.shape[1], t.shape[0]),
              "vrhip_upload_texture")

    def useBRDF(self, v: bool) -> None:
        self._need_ctx()
        check(self._lib.vrhip_use_brdf(self._ctx, int(bool(v))), "vrhip_use_brdf")

    def useExampleSphere(self, v: bool) -> None:
        self._need_ctx()
        check(self._lib.vrhip_use_example_sphere(self._ctx, int(bool(v))), "vrhip_use_example_sphere")

    def useCornellBox(self, v: bool) -> None:
        self._need_ctx()
        check(self._lib.vrhip_use_cornell_box(self._ctx, int(bool(v))), "vrhip_use_cornell_box")

    def set_strict_traversal(self, strict: bool) -> None:
        """True: visit every box the ray pierces, exactly like the reference."""
        check(self._lib.vrhip_set_strict_traversal(self._need_ctx(), int(bool(strict))), "vrhip_set_strict_traversal")

    def clearBuffer(self) -> None:
        self._need_ctx()
        check(self._lib.vrhip_clear(self._ctx), "vrhip_clear")

    def loadBRDF(self, brdf) -> bool:
        """Returns False for None, like vRendererCuda::loadBRDF (src/vRendererCuda.cpp:413-437)."""
        if brdf is None:
            return False
        self._need_ctx()
        b = _f32(brdf).reshape(-1)
        check(self._lib.vrhip_upload_brdf(self._ctx, fptr(b), b.size), "vrhip_upload_brdf")
        return True

    def getFrameCount(self) -> int:
        self._need_ctx()
        n = ctypes.c_uint32(0)
        check(self._lib.vrhip_frame_count(self._ctx, ctypes.byref(n)), "vrhip_frame_count")
        return n.value

    # -- non-virtual vRenderer members (include/vRenderer.h:139-151) -----
    def setFresnelCoef(self, v: float) -> None:
        self.m_fresnelCoef = float(v)
        self._need_ctx()
        check(self._lib.vrhip_set_fresnel(self._ctx, self.m_fresnelCoef, self.m_fresnelPow), "vrhip_set_fresnel")
        self.clearBuffer()

    def setFresnelPower(self, v: float) -> None:
        self.m_fresnelPow = float(v)
        self._need_ctx()
        check(self._lib.vrhip_set_fresnel(self._ctx, self.m_fresnelCoef, self.m_fresnelPow), "vrhip_set_fresnel")
        self.clearBuffer()

    def setCamera(self, cam: Camera) -> None:
        self._camera = cam
        self.updateCamera()

    # -- read-back / multi-GPU helpers ------------------------------------
    def read_accum(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.float32)
        check(self._lib.vrhip_read_accum(self._need_ctx(), fptr(out)), "vrhip_read_accum")
        return out

    def read_rgba8(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.uint8)
        check(self._lib.vrhip_read_rgba8(self._need_ctx(), out.ctypes.data_as(_native._u8)), "vrhip_read_rgba8")
        return out

    def read_depth8(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.uint8)
        check(self._lib.vrhip_read_depth8(self._need_ctx(), out.ctypes.data_as(_native._u8)), "vrhip_read_depth8")
        return out

    def set_stream(self, stream_handle) -> None:
        check(self._lib.vrhip_set_stream(self._need_ctx(), ctypes.c_void_p(stream_handle)), "vrhip_set_stream")

    def get_stream(self) -> int:
        """hipStream_t the context enqueues on (as an integer handle)."""
        return int(self._lib.vrhip_get_stream(self._need_ctx()) or 0)

    def sync(self) -> None:
        check(self._lib.vrhip_sync(self._need_ctx()), "vrhip_sync")

    def set_tiling(self, rank: int, n_ranks: int) -> None:
        check(self._lib.vrhip_set_tiling(self._need_ctx(), rank, n_ranks), "vrhip_set_tiling")

    def set_path_split(self, groups: int) -> None:
        """Path groups per pixel per launch (0 = automatic, 1 = off); results are unchanged."""
        check(self._lib.vrhip_set_path_split(self._need_ctx(), groups), "vrhip_set_path_split")

    def set_overlap(self, mode: int) -> None:
        """Overlap of consecutive render launches: 1 always, 0 never, -1 automatic (vrhip_set_overlap)."""
        check(self._lib.vrhip_set_overlap(self._need_ctx(), int(mode)), "vrhip_set_overlap")

    def device_group(self) -> list:
        """The devices this renderer runs on (lead first; vrhip_device_group)."""
        n = ctypes.c_uint32(0)
        check(self._lib.vrhip_device_group(self._need_ctx(), ctypes.byref(n), None), "vrhip_device_group")
        devs = (ctypes.c_int * n.value)()
        check(self._lib.vrhip_device_group(self._ctx, ctypes.byref(n), devs), "vrhip_device_group")
        return list(devs)

    def set_service(self, mode: int) -> None:
        """Render service sessions (consecutive launches on one persistent
        kernel): 1 always, 0 never, -1 automatic (vrhip_set_service)."""
        check(self._lib.vrhip_set_service(self._need_ctx(), int(mode)), "vrhip_set_service")

    def set_kernel_timing(self, on: bool) -> None:
        """HIP events around calls and launches for kernel_stats /
        last_kernel_ms (vrhip_set_kernel_timing; off saves ~8 us per
        synchronous one-frame call)."""
        check(self._lib.vrhip_set_kernel_timing(self._need_ctx(), int(bool(on))), "vrhip_set_kernel_timing")

    def set_sync_flag(self, on: bool) -> None:
        """vrhip_sync by the finish pass's completion flag after one-launch
        calls (vrhip_set_sync_flag; on by default)."""
        check(self._lib.vrhip_set_sync_flag(self._need_ctx(), int(bool(on))), "vrhip_set_sync_flag")

    def sync_info(self) -> dict:
        """Synchronisations since creation, by how they ended (vrhip_sync_info)."""
        c = (ctypes.c_uint64 * 2)()
        check(self._lib.vrhip_sync_info(self._need_ctx(), c), "vrhip_sync_info")
        return {"flag": int(c[0]), "stream": int(c[1])}

    def set_service_timing(self, idle_us: int = 0, post_window_us: int = 0, post_delay_us: int = 0) -> None:
        """Test hook (vrhip_set_service_timing): the session kernel's idle
        limit, the host's post window and a host delay before each post
        (0 = default)."""
        check(self._lib.vrhip_set_service_timing(self._need_ctx(), int(idle_us), int(post_window_us),
                                                 int(post_delay_us)), "vrhip_set_service_timing")

    def set_service_budget(self, nbytes: int = 0) -> None:
        """Scratch budget of the render service's launch slots (0: default)."""
        check(self._lib.vrhip_set_service_budget(self._need_ctx(), int(nbytes)), "vrhip_set_service_budget")

    def service_refused(self) -> int:
        """Launches that met a retiring session kernel and took the launch path."""
        n = ctypes.c_uint64(0)
        check(self._lib.vrhip_service_stats(self._need_ctx(), ctypes.byref(n)), "vrhip_service_stats")
        return int(n.value)

    def service_info(self) -> dict:
        """Render-service counts since creation (vrhip_service_info)."""
        c = (ctypes.c_uint64 * 5)()
        check(self._lib.vrhip_service_info(self._need_ctx(), c), "vrhip_service_info")
        return {"refused": int(c[0]), "sessions": int(c[1]), "served": int(c[2]), "deferred_gathers": int(c[3]),
                "alloc_fallbacks": int(c[4])}

    def owned_pixels(self) -> int:
        """Pixels this rank renders (256 per owned 16x16 tile)."""
        n = ctypes.c_uint32(0)
        check(self._lib.vrhip_owned_pixels(self._need_ctx(), ctypes.byref(n)), "vrhip_owned_pixels")
        return n.value

    def pack_tiles(self, what: int, dst_ptr: int) -> None:
        check(self._lib.vrhip_pack_tiles(self._need_ctx(), what, ctypes.c_void_p(dst_ptr)), "vrhip_pack_tiles")

    def unpack_tiles(self, what: int, src_ptr: int, n_ranks: int, stride_bytes: int = 0) -> None:
        check(self._lib.vrhip_unpack_tiles(self._need_ctx(), what, ctypes.c_void_p(src_ptr), n_ranks, stride_bytes),
              "vrhip_unpack_tiles")

    # -- multi-GPU tile gather over RCCL (vrhip_comm_*) --------------------
    def comm_init(self, rank: int, n_ranks: int, unique_id: bytes) -> None:
        """Join the n_ranks RCCL communicator named by unique_id (from
        comm_unique_id() on rank 0) and take tiles rank, rank+n, ... ."""
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f"unique id must be {COMM_ID_BYTES} bytes")
        buf = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        check(self._lib.vrhip_comm_init(self._need_ctx(), rank, n_ranks, buf), "vrhip_comm_init")

    def comm_gather(self, what: int) -> None:
        """Pack, ncclGather to rank 0, unpack on rank 0 (enqueued on the context stream)."""
        check(self._lib.vrhip_comm_gather(self._need_ctx(), int(what)), "vrhip_comm_gather")

    def comm_destroy(self) -> None:
        check(self._lib.vrhip_comm_destroy(self._need_ctx()), "vrhip_comm_destroy")

    def render_counted(self, frames: int = 1, times=None, time_seed=None) -> dict:
        """Render through the counting kernel variant; returns the event counts."""
        arr = None
        if times is not None:
            arr = (ctypes.c_uint32 * frames)(*[int(t) & 0xFFFFFFFF for t in times])
        if time_seed is None:
            time_seed = self.default_time if self.default_time is not None else int(_time.time() * 1000)
        c = (ctypes.c_uint64 * 8)()
        check(self._lib.vrhip_render_counted(self._need_ctx(), frames, arr, int(time_seed) & 0xFFFFFFFF, c),
              "vrhip_render_counted")
        names = ["rays", "node_visits", "slot_reads", "tri_tests", "attr_bytes", "tex_fetches", "hdr_fetches",
                 "brdf_fetches"]
        return {n: int(v) for n, v in zip(names, c)}

    def render_profiled(self, frames: int = 1, times=None, time_seed=None) -> dict:
        """Render through the instrumented production kernels (vrhip_render_profiled):
        the same work as render(), plus counts of the memory operations it issues."""
        arr = None
        if times is not None:
            arr = (ctypes.c_uint32 * frames)(*[int(t) & 0xFFFFFFFF for t in times])
        if time_seed is None:
            time_seed = self.default_time if self.default_time is not None else int(_time.time() * 1000)
        c = (ctypes.c_uint64 * 17)()
        check(self._lib.vrhip_render_profiled(self._need_ctx(), frames, arr, int(time_seed) & 0xFFFFFFFF, c),
              "vrhip_render_profiled")
        names = ["rays", "node_visits", "slot_reads", "tri_tests", "attr_bytes", "tex_fetches", "hdr_fetches",
                 "brdf_fetches", "node_visits_lds", "tri_loads", "mesh_hits", "nmap_hits", "lane_loads_b128",
                 "lane_loads_b96", "lane_loads_b64", "lane_loads_b32", "shared_miss_paths"]
        return {n: int(v) for n, v in zip(names, c)}

    def kernel_stats(self, reset: bool = False):
        ms = ctypes.c_double(0)
        n = ctypes.c_uint64(0)
        check(self._lib.vrhip_kernel_stats(self._need_ctx(), ctypes.byref(ms), ctypes.byref(n), int(reset)),
              "vrhip_kernel_stats")
        return float(ms.value), int(n.value)

    def last_launch_info(self) -> dict:
        """Shape of the last production launch (vrhip_last_launch_info)."""
        sp, us, kd = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(self._lib.vrhip_last_launch_info(self._need_ctx(), ctypes.byref(sp), ctypes.byref(us), ctypes.byref(kd)),
              "vrhip_last_launch_info")
        return {"split": int(sp.value), "use_scratch": int(us.value),
                "kind": ("render_kernel", "path_pool", "service", "path_pool_graph")[min(int(kd.value), 3)]}

    def device_buffers(self):
        a, r, d = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(self._lib.vrhip_device_buffers(self._need_ctx(), ctypes.byref(a), ctypes.byref(r), ctypes.byref(d)),
              "vrhip_device_buffers")
        return a.value, r.value, d.value

    def last_kernel_ms(self) -> float:
        ms = ctypes.c_float(0)
        check(self._lib.vrhip_last_kernel_ms(self._need_ctx(), ctypes.byref(ms)), "vrhip_last_kernel_ms")
        return float(ms.value)

    def bvh_info(self):
        d, n, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(self._lib.vrhip_bvh_info(self._need_ctx(), ctypes.byref(d), ctypes.byref(n), ctypes.byref(s)),
              "vrhip_bvh_info")
        return d.value, n.value, s.value

    def _need_ctx(self):
        if not self._ctx:
            raise VRHIPError(-1, "VRendererHIP", "init() has not been called")
        return self._ctx

    def __del__(self):
        try:
            self.cleanUp()
        except Exception:
            pass


def selftest_math(fn: int, a, b=None, device: int = 0) -> np.ndarray:
    """Evaluate the device libm (0 sin, 1 cos, 2 acos, 3 atan2, 4 pow, 5 fmin, 6 fmax, 7 f2i, 8 d2i(a * b), 9 f2u8,
    10 sqrt_exact, 11 inv_sqrt_exact; fn | 0x100: functions 0..4 in the sphere kernels' constant form).  Element
    i runs on lane i % 64 of wave i / 64 (include/vrhip.h)."""
    a = _f32(a).reshape(-1)
    b = _f32(np.zeros_like(a) if b is None else b).reshape(-1)
    out = np.zeros_like(a)
    check(_native.lib().vrhip_selftest_math(device, fn, fptr(a), fptr(b), fptr(out), a.size), "vrhip_selftest_math")
    return out


def selftest_brdf(table, frames, device: int = 0) -> np.ndarray:
    """The shading step's BRDF lookup on frames [n, 4, 4] (refl, cur, normal,
    tangent) against a planar MERL table of 3*90*90*180 floats
    (vrhip_selftest_brdf): [n, 4] float32."""
    t = _f32(table).reshape(-1)
    f = _f32(frames).reshape(-1, 16)
    out = np.zeros((f.shape[0], 4), np.float32)
    check(_native.lib().vrhip_selftest_brdf(device, fptr(t), t.size, fptr(f), f.shape[0], fptr(out)),
          "vrhip_selftest_brdf")
    return out


def selftest_half_box(values, device: int = 0):
    """The device BVH builder's outward fp32 -> fp16 box rounding
    (vrhip_selftest_half_box): (down, up) as uint16 bit patterns."""
    a = _f32(values).reshape(-1)
    down = np.zeros(a.size, np.uint16)
    up = np.zeros(a.size, np.uint16)
    check(_native.lib().vrhip_selftest_half_box(device, fptr(a), a.size, down.ctypes.data_as(_native._u16),
                                                up.ctypes.data_as(_native._u16)), "vrhip_selftest_half_box")
    return down, up


def selftest_rcp(lo_bits: int, hi_bits: int, device: int = 0):
    """Exhaustively compare the kernels' reciprocal with IEEE 1/x over the float
    bit patterns [lo_bits, hi_bits) and their negations: (mismatches, first_bad)."""
    n = ctypes.c_uint64(0)
    first = ctypes.c_uint32(0)
    check(_native.lib().vrhip_selftest_rcp(device, lo_bits, hi_bits, ctypes.byref(n), ctypes.byref(first)),
          "vrhip_selftest_rcp")
    return int(n.value), int(first.value)


def selftest_tonemap(lo_bits: int = 0, hi_bits: int = 0x3F800001, device: int = 0):
    """Exhaustively compare the kernels' table tonemap byte with the f64
    pow byte over the float bit patterns [lo_bits, hi_bits) (+ -0.0):
    (mismatches, first_bad)."""
    n = ctypes.c_uint64(0)
    first = ctypes.c_uint32(0)
    check(_native.lib().vrhip_selftest_tonemap(device, lo_bits, hi_bits, ctypes.byref(n), ctypes.byref(first)),
          "vrhip_selftest_tonemap")
    return int(n.value), int(first.value)


def selftest_sqrt(lo_bits: int, hi_bits: int, device: int = 0):
    """Exhaustively compare the kernels' square root with sqrtf over the float
    bit patterns [lo_bits, hi_bits): (mismatches, first_bad)."""
    n = ctypes.c_uint64(0)
    first = ctypes.c_uint32(0)
    check(_native.lib().vrhip_selftest_sqrt(device, lo_bits, hi_bits, ctypes.byref(n), ctypes.byref(first)),
          "vrhip_selftest_sqrt")
    return int(n.value), int(first.value)


def microbench_vmem(width_bytes: int, distinct: int, device: int = 0) -> float:
    """Lane loads per second of the device's vector-memory gather path (vrhip_microbench_vmem)."""
    r = ctypes.c_double(0)
    check(_native.lib().vrhip_microbench_vmem(device, width_bytes, distinct, ctypes.byref(r)), "vrhip_microbench_vmem")
    return float(r.value)


COMM_ID_BYTES = 128    # VRHIP_COMM_ID_BYTES


def comm_unique_id() -> bytes:
    """A fresh RCCL communicator id (vrhip_comm_unique_id), to hand to every rank."""
    buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
    check(_native.lib().vrhip_comm_unique_id(buf), "vrhip_comm_unique_id")
    return bytes(buf)


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = _native.lib().vrhip_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0
