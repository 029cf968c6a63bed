"""Helpers of test_gpu_streams.py: a bounded device-side delay with its
calibration, an asynchronous copy from a raw device pointer on a given stream,
the two ways a caller comes to share the context stream, the render sequences
of parts A and B and the query cases of parts C and D, each with a valid decoy
input A and the real input B.

Nothing here waits on the host for longer than a delay lasts: a delay is one
torch.cuda._sleep of about DELAY_MS, never more than MAX_DELAY_MS, and every
delay a test relies on is measured with events and checked (check_delays)."""
import ctypes
import functools
import os
import re
import time

import numpy as np

import denoise_cases as dn
import device_mesh_cases as dm
from vrenderer_pathtracer_amd import VRendererHIP, scenes, tiles
from vrenderer_pathtracer_amd._native import check

DELAY_MS = 30.0          # what a delay aims at
MIN_DELAY_MS = 20.0      # what it must have lasted for the test that used it to mean anything
MAX_DELAY_MS = 100.0     # never more than this in one call
MAX_HOST_PATH_MS = MIN_DELAY_MS / 10.0   # the host's way from enqueuing a delay to the library's launch
N = 1000                 # rays, records, probes: not a multiple of 64
PLACEMENTS = ("set", "get")


# ---- the HIP runtime the process has loaded ------------------------------------------
@functools.lru_cache(maxsize=None)
def hip():
    """ctypes handle of the libamdhip64 this process has ALREADY mapped (torch's:
    see the note at the top of _native.py), found in /proc/self/maps and opened
    by that very path, so the loader hands back the mapped copy and no second
    runtime comes in."""
    import torch  # noqa: F401  (maps the runtime)
    paths = []
    with open("/proc/self/maps") as f:
        for line in f:
            m = re.search(r"(/\S*libamdhip64\.so[^/\s]*)$", line.strip())
            if m and m.group(1) not in paths:
                paths.append(m.group(1))
    real = sorted({os.path.realpath(p) for p in paths})
    assert len(real) == 1, f"expected one loaded libamdhip64, found {real}"
    lib = ctypes.CDLL(paths[0])
    lib.hipMemcpyAsync.restype = ctypes.c_int
    lib.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return lib


HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def copy_on(stream, dst_tensor, src_ptr, nbytes):
    """Asynchronous device-to-device copy of nbytes from the raw pointer
    src_ptr into dst_tensor, enqueued on the torch stream `stream`."""
    assert dst_tensor.is_contiguous() and dst_tensor.numel() * dst_tensor.element_size() >= nbytes
    e = hip().hipMemcpyAsync(dst_tensor.data_ptr(), src_ptr, nbytes, HIP_MEMCPY_DEVICE_TO_DEVICE, stream.cuda_stream)
    assert e == 0, f"hipMemcpyAsync: error {e}"


# ---- the delay -------------------------------------------------------------------------
_issued = []             # (start, end) events of the delays since the last check


@functools.lru_cache(maxsize=None)
def calibration():
    """Cycles of torch.cuda._sleep per millisecond, from torch events: probes
    grow from 200,000 cycles (2 ms on a 100 MHz counter, 0.1 ms on a 2 GHz one)
    by at most 10x a step until one lasts 2 ms; none can exceed about 20 ms.
    Returns dict(cycles_per_ms, delay_cycles, probes=[(cycles, ms), ...])."""
    import torch
    s = torch.cuda.Stream(0)
    probes = []
    cycles = 200_000
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)                               # load the kernel
        s.synchronize()
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            torch.cuda._sleep(cycles)
            e1.record(s)
            s.synchronize()
            ms = e0.elapsed_time(e1)
            probes.append((cycles, ms))
            if ms >= 2.0:
                break
            cycles = int(cycles * min(10.0, 4.0 / max(ms, 1e-3)))
    cycles, ms = probes[-1]
    assert ms >= 2.0, f"torch.cuda._sleep could not be calibrated: {probes}"
    per_ms = cycles / ms
    return {"cycles_per_ms": per_ms, "delay_cycles": int(per_ms * DELAY_MS), "probes": probes}


def delay(stream):
    """About DELAY_MS of busy kernel on the torch stream `stream`, between two
    timing events that check_delays reads."""
    import torch
    cal = calibration()
    cycles = cal["delay_cycles"]
    assert cycles <= cal["cycles_per_ms"] * MAX_DELAY_MS
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        torch.cuda._sleep(cycles)
        e1.record(stream)
    _issued.append((e0, e1))
    return e0, e1


def forget_delays():
    del _issued[:]


def check_delays(expected=None):
    """After the test's final synchronisation: every delay since the last
    check lasted MIN_DELAY_MS or more (a condition of the test, not a
    measurement: a delay that did not bite proves nothing).  Returns the ms."""
    ms = [e0.elapsed_time(e1) for e0, e1 in _issued]
    forget_delays()
    if expected is not None:
        assert len(ms) == expected, f"{len(ms)} delays issued, {expected} expected"
    assert ms, "the test relied on no delay"
    assert min(ms) >= MIN_DELAY_MS, f"a delay lasted {min(ms):.2f} ms (< {MIN_DELAY_MS} ms): {ms}"
    assert max(ms) <= 2.0 * MAX_DELAY_MS, f"a delay lasted {max(ms):.2f} ms: {ms}"
    return ms


# ---- who owns the stream ---------------------------------------------------------------
class Shared:
    """The context stream as a torch stream, in one of the two placements:
    "set": a torch stream given to the context (vrhip_set_stream);
    "get": the context's own stream wrapped (vrhip_get_stream).
    Keep the object alive until the renderer's cleanUp()."""

    def __init__(self, r, placement):
        import torch
        self.placement = placement
        if placement == "set":
            self.s = torch.cuda.Stream(0)
            r.set_stream(self.s.cuda_stream)
        elif placement == "get":
            self.s = torch.cuda.ExternalStream(r.get_stream(), device=torch.device("cuda", 0))
        else:
            raise ValueError(placement)


# ---- scenes, sequences, renders ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    """The smallest scenes that still take every path (never written)."""
    if name == "C2":
        return scenes.make_scene("C2", 64, 48, knot=(40, 20))     # 1,600 triangles, Cornell path pool
    if name == "C3":
        return scenes.make_scene("C3", 96, 64)                    # HDRI mesh, sparse launches
    if name == "C4":
        return scenes.make_scene("C4", 96, 64)                    # sphere scene, render_kernel
    raise ValueError(name)


# calls: frames per vrhip_render; sync: vrhip_sync after every call; kind: what vrhip_last_launch_info must
# show on a mesh scene (a sphere scene always shows render_kernel)
SEQUENCES = {
    # part A: every launch kind the suite knows
    "multi3": dict(calls=[3], sync=True, kind="path_pool"),
    "sync1x6": dict(calls=[1] * 6, sync=True, kind="path_pool"),
    "lanes1x6": dict(calls=[1] * 6, sync=False, overlap=1, service=0, kind="path_pool"),
    "service213": dict(calls=[2, 1, 3], sync=False, service=1, kind="service"),
    "graph1x6": dict(calls=[1] * 6, sync=True, graph=True, kind="path_pool_graph"),
    "rank1of3": dict(calls=[3], sync=True, tiling=(1, 3), kind="path_pool"),
    # part B: all unsynchronised
    "b_multi3": dict(calls=[3], sync=False),
    "b_1x3_overlap1": dict(calls=[1, 1, 1], sync=False, overlap=1),
    "b_1x3_overlap0": dict(calls=[1, 1, 1], sync=False, overlap=0),
    "b_2x2_auto": dict(calls=[2, 2], sync=False),                 # the default service mode
    "b_2x2_direct": dict(calls=[2, 2], sync=False, split=1),      # a sphere scene's direct mode: no finish pass
    "b_rank1of3": dict(calls=[2, 1], sync=False, tiling=(1, 3)),
    "b_2x2_service": dict(calls=[2, 2], sync=False, service=1, reclose=True),
}


def new_renderer(sc, seq):
    """A renderer with the scene loaded and the sequence's settings applied."""
    old = os.environ.get("VRHIP_GRAPH")
    if seq.get("graph"):
        os.environ["VRHIP_GRAPH"] = "1"
    try:
        r = VRendererHIP(0)
        scenes.load_into(r, sc)                # (init() creates the context, which reads VRHIP_GRAPH)
    finally:
        if seq.get("graph"):
            if old is None:
                del os.environ["VRHIP_GRAPH"]
            else:
                os.environ["VRHIP_GRAPH"] = old
    if seq.get("graph"):
        r.set_kernel_timing(False)
    if "service" in seq:
        r.set_service(seq["service"])
    if "overlap" in seq:
        r.set_overlap(seq["overlap"])
    if "split" in seq:
        r.set_path_split(seq["split"])
    if "tiling" in seq:
        r.set_tiling(*seq["tiling"])
    return r


def run_calls(r, sc, seq, first=0):
    """The sequence's render calls, frame i of the run with time sc["time"] + i;
    returns the launch kind after every call."""
    t = sc["time"] + first
    kinds = []
    for n in seq["calls"]:
        r.render(frames=n, times=[t + k for k in range(n)], sync=seq["sync"])
        kinds.append(r.last_launch_info()["kind"])
        t += n
    return kinds


def read_all(r):
    return {"accum": r.read_accum(), "rgba8": r.read_rgba8(), "depth8": r.read_depth8(), "frames": r.getFrameCount()}


@functools.lru_cache(maxsize=None)
def untouched(scene_name, seq_name):
    """The sequence on a context that never handed anything out, read back
    through the library (never written)."""
    sc, seq = scene(scene_name), SEQUENCES[seq_name]
    r = new_renderer(sc, seq)
    kinds = run_calls(r, sc, seq)
    out = read_all(r)
    out["kinds"] = kinds
    r.cleanUp()
    return out


@functools.lru_cache(maxsize=None)
def oracle_images(scene_name, frames):
    import pyoracle as po
    sc = scene(scene_name)
    a, rgba, d, _ = po.render(sc, frames=frames, times=[sc["time"] + k for k in range(frames)], libm=po.LIBM_PORTABLE)
    return {"accum": a, "rgba8": rgba, "depth8": d}


def owned_pixels(w, h, rank, n_ranks):
    """Linear pixel indices of the rank's tiles."""
    return tiles.owned_pixels(w, h, rank, n_ranks).astype(np.int64)


def differing(a, b):
    """Pixels (rows) whose words differ, as a count; float32 compares as uint32."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    d = a != b
    return int(d.reshape(-1, d.shape[-1]).any(-1).sum()) if d.ndim > 1 else int(d.sum())


# ---- parts C and D: one case per entry point, decoy A and input B for every device input ----
def words(t):
    """A device tensor as host uint32 words (the stream it was written on has been waited for)."""
    a = t.detach().cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else a.dtype).copy()


def same(a, b):
    return a.shape == b.shape and bool(np.array_equal(a, b))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


KNOT = scenes.torus_knot(40, 20)             # 800 vertices, 1,600 triangles
GRID_W, GRID_H = 40, 25                      # 1,000 cells
PROBE_DIRS = 65                              # one block and a one-lane tail
DENOISE = dict(passes=3)


def _rays(seed):
    rng = np.random.default_rng(seed)
    o = (rng.uniform(-15.0, 15.0, (N, 3)) + np.array([0.0, 0.0, 150.0])).astype(np.float32)
    d = (rng.uniform(-45.0, 45.0, (N, 3)) - o).astype(np.float32)
    return o, d


def _units(rng, n):
    v = rng.normal(0.0, 1.0, (n, 3))
    return (v / np.sqrt((v * v).sum(-1, keepdims=True))).astype(np.float32)


def _seeds(rng, n):
    return rng.integers(0, 2 ** 32, (n, 2), dtype=np.uint64).astype(np.uint32).view(np.int32)


def scene_context():
    """C2 with its mesh rebuilt on the device from KNOT (so that refits and
    vrhip_surface_at's triangle numbers apply), on its own stream."""
    r = VRendererHIP(0)
    scenes.load_into(r, scene("C2"))
    dm.device_build(r, KNOT)
    return r


def bare_context():
    return dm.fresh()


@functools.lru_cache(maxsize=None)
def _surface_records(which):
    """(N, 28) float32 records of ray set `which` (0: A, 1: B) in the query scene."""
    import torch
    o, d = _rays(101 + which)
    r = scene_context()
    rec = r.traceSurface(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())["record"].cpu().numpy()
    r.cleanUp()
    return rec


class Case:
    """name; context(): a renderer on its own stream; data(): {input: (A, B)}
    numpy arrays, the device inputs that can be pending, plus {input: array}
    for the ones that cannot; raw(r, t) / wrapped(r, t): the call through the
    C ABI / through VRendererHIP on the dict t of device tensors, returning
    host uint32 words."""

    def __init__(self, name, context, data, raw, wrapped, method):
        self.name, self.context, self._data, self.raw, self.wrapped, self.method = name, context, data, raw, wrapped, method

    @functools.lru_cache(maxsize=None)
    def data(self):
        return self._data()


def _lib(r):
    return r._lib


def _trace_rays_data():
    (oa, da), (ob, db) = _rays(1), _rays(2)
    rng = np.random.default_rng(3)
    return {"origins": (oa, ob), "dirs": (da, db),
            "tmax": (np.full(N, 1e20, np.float32), rng.uniform(0.5, 1.1, N).astype(np.float32))}


def _trace_rays_raw(r, t):
    import torch
    rec = torch.empty((N, 4), dtype=torch.int32, device="cuda:0")
    check(_lib(r).vrhip_trace_rays(r._ctx, _p(t["origins"]), _p(t["dirs"]), _p(t["tmax"]), N, 0, _p(rec)), "vrhip_trace_rays")
    return words(rec)


def _trace_rays_wrapped(r, t):
    h = r.traceRays(t["origins"], t["dirs"], t["tmax"])
    return np.stack([words(h["t"]), h["prim"].cpu().numpy().astype(np.uint32), words(h["u"]), words(h["v"])], -1)


def _radiance_data():
    (oa, da), (ob, db) = _rays(11), _rays(12)
    rng = np.random.default_rng(13)
    return {"origins": (oa, ob), "dirs": (da, db), "seeds": (_seeds(rng, N), _seeds(rng, N))}


def _radiance_raw(r, t):
    import torch
    out = torch.empty((N, 4), dtype=torch.float32, device="cuda:0")
    check(_lib(r).vrhip_trace_radiance(r._ctx, _p(t["origins"]), _p(t["dirs"]), _p(t["seeds"]), N, 2, _p(out)),
          "vrhip_trace_radiance")
    return words(out)


def _radiance_wrapped(r, t):
    return words(r.traceRadiance(t["origins"], t["dirs"], t["seeds"], samples=2))


def _surface_data():
    (oa, da), (ob, db) = _rays(21), _rays(22)
    return {"origins": (oa, ob), "dirs": (da, db)}


def _surface_raw(r, t):
    import torch
    rec = torch.empty((N, 28), dtype=torch.float32, device="cuda:0")
    check(_lib(r).vrhip_trace_surface(r._ctx, _p(t["origins"]), _p(t["dirs"]), N, _p(rec)), "vrhip_trace_surface")
    return words(rec)


def _surface_wrapped(r, t):
    return words(r.traceSurface(t["origins"], t["dirs"])["record"])


def _shade_data():
    rng = np.random.default_rng(33)
    return {"records": (_surface_records(0), _surface_records(1)), "dirs": (_rays(101)[1], _rays(102)[1]),
            "seeds": (_seeds(rng, N), _seeds(rng, N))}


def _shade_raw(r, t):
    import torch
    out = torch.empty((N, 4), dtype=torch.float32, device="cuda:0")
    check(_lib(r).vrhip_shade_surface(r._ctx, _p(t["records"]), _p(t["dirs"]), _p(t["seeds"]), N, 2, _p(out)),
          "vrhip_shade_surface")
    return words(out)


def _shade_wrapped(r, t):
    return words(r.shadeSurface(t["records"], t["dirs"], t["seeds"], samples=2))


def _probe_data():
    rng = np.random.default_rng(41)
    k = PROBE_DIRS
    return {"points": (rng.uniform(-40.0, 40.0, (N, 3)).astype(np.float32), rng.uniform(-40.0, 40.0, (N, 3)).astype(np.float32)),
            "dirs": (_units(rng, k), _units(rng, k)),
            "weights": (rng.uniform(0.1, 0.3, k).astype(np.float32), rng.uniform(0.1, 0.3, k).astype(np.float32)),
            "probe_seeds": _seeds(rng, N), "dir_seeds": _seeds(rng, k)}


def _probe_raw(r, t):
    import torch
    out = torch.empty((N, 28), dtype=torch.float32, device="cuda:0")
    check(_lib(r).vrhip_probe_sh(r._ctx, _p(t["points"]), _p(t["dirs"]), _p(t["weights"]), _p(t["probe_seeds"]),
                                 _p(t["dir_seeds"]), N, PROBE_DIRS, 1, _p(out)), "vrhip_probe_sh")
    return words(out)


def _probe_wrapped(r, t):
    return words(r.probeSH(t["points"], t["dirs"], t["weights"], t["probe_seeds"], t["dir_seeds"], samples=1))


def _irradiance_data():
    rng = np.random.default_rng(51)
    return {"sh": (rng.normal(0.0, 1.0, (N, 28)).astype(np.float32), rng.normal(0.0, 1.0, (N, 28)).astype(np.float32)),
            "normals": (_units(rng, N), _units(rng, N))}


def _irradiance_raw(r, t):
    import torch
    out = torch.empty((N, 4), dtype=torch.float32, device="cuda:0")
    check(_lib(r).vrhip_sh_irradiance(r._ctx, _p(t["sh"]), N, None, _p(t["normals"]), N, _p(out)), "vrhip_sh_irradiance")
    return words(out)


def _irradiance_wrapped(r, t):
    return words(r.shIrradiance(t["sh"], t["normals"]))


def _surface_at_data():
    rng = np.random.default_rng(61)
    n_tris = len(KNOT["tris"])
    return {"prims": (rng.integers(0, n_tris, N).astype(np.int32), rng.integers(0, n_tris, N).astype(np.int32)),
            "bary": (rng.uniform(0.0, 0.5, (N, 2)).astype(np.float32), rng.uniform(0.0, 0.5, (N, 2)).astype(np.float32))}


def _surface_at_raw(r, t):
    import torch
    rec = torch.empty((N, 28), dtype=torch.float32, device="cuda:0")
    check(_lib(r).vrhip_surface_at(r._ctx, _p(t["prims"]), _p(t["bary"]), N, _p(rec)), "vrhip_surface_at")
    return words(rec)


def _surface_at_wrapped(r, t):
    return words(r.surfaceAt(t["prims"], t["bary"])["record"])


def _denoise_data():
    ca, ga = dn.grid(GRID_W, GRID_H)
    cb, gb = dn.grid(GRID_H, GRID_W)                      # another draw of as many cells
    return {"color": (np.array(ca), np.array(cb).reshape(GRID_H, GRID_W, 4)),
            "guides": (np.array(ga).view(np.float32), np.array(gb).view(np.float32))}


def _denoise_raw(in_place):
    def call(r, t):
        import torch
        from vrenderer_pathtracer_amd import _native
        out = t["color"] if in_place else torch.empty((GRID_H, GRID_W, 4), dtype=torch.float32, device="cuda:0")
        prm = r._denoise_params(DENOISE["passes"], r.DENOISE_DEFAULTS["sigma_color"], r.DENOISE_DEFAULTS["sigma_position"],
                                r.DENOISE_DEFAULTS["normal_power_log2"], True)
        assert isinstance(prm, _native.DenoiseParams)
        check(_lib(r).vrhip_denoise(r._ctx, _p(t["color"]), _p(t["guides"]), GRID_W, GRID_H, ctypes.byref(prm), _p(out)),
              "vrhip_denoise")
        return words(out)
    return call


def _denoise_wrapped(in_place):
    def call(r, t):
        return words(r.denoise(t["color"], t["guides"], passes=DENOISE["passes"], out=t["color"] if in_place else None))
    return call


def _mesh_words(r):
    flat = r.export_mesh_flat()
    return np.concatenate([np.asarray(flat[k], np.float32).reshape(-1).view(np.uint32) for k in ("bvh", "verts", "normals")])


def _refit_data():
    P = KNOT["positions"]
    return {"positions": (dm.deform(P, 0.03), dm.deform(P, 0.05, (5, 3, -4)))}


def _refit_raw(r, t):
    nv = int(t["positions"].shape[0])
    check(_lib(r).vrhip_refit_mesh_device(r._ctx, _p(t["positions"]), None, None, nv), "vrhip_refit_mesh_device")
    return _mesh_words(r)


def _refit_wrapped(r, t):
    r.refitMeshDevice(t["positions"])
    return _mesh_words(r)


def _upload_data():
    """The index array is a fixed input, complete before every call: a stale
    index is the one decoy that could read out of range."""
    P, Nm = KNOT["positions"].astype(np.float32), KNOT["normals"].astype(np.float32)
    return {"positions": (P, dm.deform(P)), "normals": (Nm, np.ascontiguousarray(-np.roll(Nm, 7, 0))),
            "tris": np.ascontiguousarray(KNOT["tris"]).astype(np.int32)}


def _upload_raw(builder):
    def call(r, t):
        nv, nt = int(t["positions"].shape[0]), int(t["tris"].shape[0])
        check(_lib(r).vrhip_upload_mesh_device_ex(r._ctx, _p(t["positions"]), _p(t["normals"]), None, None, nv, _p(t["tris"]),
                                                  nt, 2, VRendererHIP.DEVICE_BUILDERS[builder]), "vrhip_upload_mesh_device_ex")
        return _mesh_words(r)
    return call


def _upload_wrapped(builder):
    def call(r, t):
        r.initMeshDevice(t["positions"], t["tris"], t["normals"], builder=builder)
        return _mesh_words(r)
    return call


CASES = {c.name: c for c in (
    Case("trace_rays", scene_context, _trace_rays_data, _trace_rays_raw, _trace_rays_wrapped, "traceRays"),
    Case("trace_radiance", scene_context, _radiance_data, _radiance_raw, _radiance_wrapped, "traceRadiance"),
    Case("trace_surface", scene_context, _surface_data, _surface_raw, _surface_wrapped, "traceSurface"),
    Case("shade_surface", scene_context, _shade_data, _shade_raw, _shade_wrapped, "shadeSurface"),
    Case("probe_sh", scene_context, _probe_data, _probe_raw, _probe_wrapped, "probeSH"),
    Case("sh_irradiance", bare_context, _irradiance_data, _irradiance_raw, _irradiance_wrapped, "shIrradiance"),
    Case("surface_at", scene_context, _surface_at_data, _surface_at_raw, _surface_at_wrapped, "surfaceAt"),
    Case("denoise", bare_context, _denoise_data, _denoise_raw(False), _denoise_wrapped(False), "denoise"),
    Case("denoise_in_place", bare_context, _denoise_data, _denoise_raw(True), _denoise_wrapped(True), "denoise"),
    Case("refit", scene_context, _refit_data, _refit_raw, _refit_wrapped, "refitMeshDevice"),
    Case("upload_morton", bare_context, _upload_data, _upload_raw("morton"), _upload_wrapped("morton"), "initMeshDevice"),
    Case("upload_sah", bare_context, _upload_data, _upload_raw("sah"), _upload_wrapped("sah"), "initMeshDevice"),
)}


def case_inputs():
    """(case name, pending input) for every device input that can be pending.
    Listed by hand so that collecting the tests needs no device."""
    return [("trace_rays", "origins"), ("trace_rays", "dirs"), ("trace_rays", "tmax"),
            ("trace_radiance", "origins"), ("trace_radiance", "dirs"), ("trace_radiance", "seeds"),
            ("trace_surface", "origins"), ("trace_surface", "dirs"),
            ("shade_surface", "records"), ("shade_surface", "dirs"), ("shade_surface", "seeds"),
            ("probe_sh", "points"), ("probe_sh", "dirs"), ("probe_sh", "weights"),
            ("sh_irradiance", "sh"), ("sh_irradiance", "normals"),
            ("surface_at", "prims"), ("surface_at", "bary"),
            ("denoise", "color"), ("denoise", "guides"), ("denoise_in_place", "color"), ("denoise_in_place", "guides"),
            ("refit", "positions"),
            ("upload_morton", "positions"), ("upload_morton", "normals"),
            ("upload_sah", "positions"), ("upload_sah", "normals")]


def device_inputs(case, decoy=None):
    """The case's inputs as fresh device tensors holding B, except `decoy`,
    which holds A; complete (the device has been waited for)."""
    import torch
    t = {}
    for k, v in case.data().items():
        a = (v[0] if k == decoy else v[1]) if isinstance(v, tuple) else v
        t[k] = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


@functools.lru_cache(maxsize=None)
def quiet(case_name, decoy, through):
    """The call's result on a quiescent context with complete inputs: all B,
    or A in `decoy` (never written).  through: "raw" or "wrapped"."""
    case = CASES[case_name]
    r = case.context()
    out = getattr(case, through)(r, device_inputs(case, decoy))
    r.cleanUp()
    out.setflags(write=False)
    return out


def pending_call(case, r, name, stream, through):
    """Decoy A in input `name`, then on `stream`: a delay, the copy of B over
    it, the call (with `stream` torch's current stream).  Returns the call's
    result.  One complete call comes first, so that the measured call
    allocates nothing (the context's scratch at first use, a block of torch's
    allocator): an allocation may wait for the device and order the pending
    copy by accident."""
    import torch
    getattr(case, through)(r, device_inputs(case, name))
    t = device_inputs(case, name)
    b = torch.from_numpy(np.ascontiguousarray(case.data()[name][1])).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        delay(stream)
        t[name].copy_(b, non_blocking=True)
        return getattr(case, through)(r, t)


def host_path_ms(r, sc, stream, tries=3):
    """The host's way from enqueuing a delay to the library's launch: the wall
    time of delay + an overwriting copy + an unsynchronised one-frame
    vrhip_render (which returns once its kernels are queued), the least of
    `tries` (the first pays for lazy loading).  The delays are waited for."""
    import torch
    a = torch.zeros(3 * N, dtype=torch.float32, device="cuda:0")
    b = torch.ones(3 * N, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    best = float("inf")
    for i in range(tries):
        with torch.cuda.stream(stream):
            t0 = time.perf_counter()
            delay(stream)
            a.copy_(b, non_blocking=True)
            r.render(frames=1, times=[sc["time"] + i], sync=False)
            best = min(best, (time.perf_counter() - t0) * 1e3)
        r.sync()
        stream.synchronize()
    return best
