#!/usr/bin/env python3
"""Rate of the ray-query kernel (VRendererHIP.traceRays, vrhip_trace_rays) on
the device-built trees, closest hit, culled walk.

  python scripts/ray_query_cost.py [--out profiles/ray_query/cost.json] [--rays 4194304] [--frames 4]

One JSON line per mesh (the 10k-triangle knot of scene C2, the 1M-triangle knot
of scene C5) and builder (morton, sah):
  coherent_mrays_s    the scene camera's primary rays at the scene's resolution
                      (cuda/src/PathTracer.cu:833-844, no jitter), pixel after
                      pixel in row-major order, repeated from the first pixel
                      until --rays rays are filled (C5 has more pixels than
                      that: its first rows)
  incoherent_mrays_s  origins uniform in the mesh's bounds, directions uniform
                      on the sphere
  *_ms_all, *_hit_share   the timed calls and the share of rays that hit
  any_hit_*           the same two ray sets as occlusion queries
Each rate is the best of 5 calls after 2 warm-up calls, timed by events
recorded on the context stream around the (synchronous) call, into a
pre-allocated result buffer.
For context only, path_kernel_mrays_s: the rays the scene's path kernels trace
per second on the same tree -- the ray count of vrhip_render_counted for
--frames frames over the kernel time (vrhip_last_kernel_ms) of the production
render of the same frames.  Those rays also shade, and their bounces are
incoherent; the two numbers are not a like-for-like comparison.
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrenderer_pathtracer_amd import VRendererHIP, scenes  # noqa: E402


def camera_rays(r, n):
    """The renderer's own camera rays (cameraRays(): cuda/src/PathTracer.cu:833-844), normalised as the camera ray is:
    (origins, dirs) of the first n pixels, row-major, wrapped."""
    o, d = r.cameraRays()
    i = torch.arange(n, device=o.device) % o.shape[0]
    d = d / d.norm(dim=1, keepdim=True)
    return o[i].contiguous(), d[i].contiguous()


def random_rays(lo, hi, n, dev, seed=7):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    o = torch.rand((n, 3), generator=g, device=dev) * (hi - lo)[None, :] + lo[None, :]
    d = torch.randn((n, 3), generator=g, device=dev)
    return o.contiguous(), (d / d.norm(dim=1, keepdim=True)).contiguous()


def time_query(r, o, d, any_hit, stream, warm=2, reps=5):
    n = o.shape[0]
    rec = torch.empty((n, 4), dtype=torch.int32, device=o.device)
    torch.cuda.synchronize()
    ms = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = r._lib.vrhip_trace_rays(r._ctx, ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(d.data_ptr()), None, n,
                                     1 if any_hit else 0, ctypes.c_void_p(rec.data_ptr()))
        e1.record(stream)
        e1.synchronize()
        assert rc == 0, rc
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    hits = int((rec[:, 1] != -1).sum()) if not any_hit else int((rec[:, 1] == 0).sum())
    return ms, hits / n


def measure(cfg, nu, nv, leaf, builder, n_rays, frames):
    dev = torch.device("cuda", 0)
    mesh = scenes.torus_knot(nu, nv)
    sc = scenes.make_scene(cfg, knot=(nu, nv))
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    pos = torch.from_numpy(np.ascontiguousarray(mesh["positions"])).to(dev)
    tris = torch.from_numpy(np.ascontiguousarray(mesh["tris"], np.int32)).to(dev)
    r.initMeshDevice(pos, tris, max_leaf_tris=leaf, builder=builder)
    stream = torch.cuda.ExternalStream(r.get_stream(), device=dev)
    out = {"scene": cfg, "knot": [nu, nv], "n_tris": int(len(mesh["tris"])), "max_leaf_tris": leaf, "builder": builder,
           "depth": r.bvh_info()[0], "walk": "culled", "n_rays": n_rays, "resolution": [sc["width"], sc["height"]]}
    sets = {"coherent": camera_rays(r, n_rays),
            "incoherent": random_rays(pos.min(0).values, pos.max(0).values, n_rays, dev)}
    for name, (o, d) in sets.items():
        for any_hit in (False, True):
            ms, share = time_query(r, o, d, any_hit, stream)
            key = ("any_hit_" if any_hit else "") + name
            out[key + "_mrays_s"] = round(n_rays / min(ms) / 1e3, 1)
            out[key + "_ms_all"] = [round(m, 4) for m in ms]
            out[key + "_hit_share"] = round(share, 4)
    times = [sc["time"] + k for k in range(frames)]
    r.clearBuffer()
    r.render(frames=frames, times=times)                       # warm-up
    best = None
    for _ in range(3):
        r.clearBuffer()
        r.render(frames=frames, times=times)
        ms = r.last_kernel_ms()
        best = ms if best is None else min(best, ms)
    r.clearBuffer()
    rays = r.render_counted(frames=frames, times=times)["rays"]
    out.update(path_kernel_frames=frames, path_kernel_rays=rays, path_kernel_ms=round(best, 4),
               path_kernel_mrays_s=round(rays / best / 1e3, 1))
    r.cleanUp()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--frames", type=int, default=4)
    a = ap.parse_args()
    lines = []
    for cfg, nu, nv, leaf in (("C2", 100, 50, 2), ("C5", 1000, 500, 4)):
        for builder in ("morton", "sah"):
            lines.append(json.dumps(measure(cfg, nu, nv, leaf, builder, a.rays, a.frames)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
