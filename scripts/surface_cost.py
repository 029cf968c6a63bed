#!/usr/bin/env python3
"""Rate of the surface query kernel (VRendererHIP.traceSurface,
vrhip_trace_surface), culled walk.

  python scripts/surface_cost.py [--out profiles/surface/cost.json] [--rays 1048576]

One JSON line per scene (C2: Cornell box + the 10k-triangle knot; C5: HDRI +
the 1M-triangle knot, both with the host-built tree the scene loads), with, for
each of two ray sets,
  camera   the scene camera's rays at the scene's resolution (cameraRays():
           the un-normalised directions, as the calls take them), pixel after
           pixel in row-major order, repeated from the first pixel until
           --rays rays are filled
  random   origins uniform in the mesh's bounds, directions uniform on the
           sphere
three rates on the same rays in the same process:
  <set>_surface_mrays_s    vrhip_trace_surface (112 B written per ray)
  <set>_radiance1_mrays_s  vrhip_trace_radiance with one path per ray (16 B)
  <set>_closest_mrays_s    vrhip_trace_rays, closest hit, the mesh only (16 B)
  *_ms_all                 the timed calls;  <set>_hit_share, <set>_mesh_share:
                           rays that hit anything / the mesh in the surface query
Each rate is rays over the best of 5 synchronous calls after 2 warm-up calls,
timed by events recorded on the context stream around the call, into a
pre-allocated result buffer.
A surface query does a subset of a one-path radiance query's work on a ray
that hits (the first intersection and one fill_hit against a whole path) and
writes seven times the bytes; surface_over_radiance1 is the ratio of the two
rates per set.  No bar is set for these rates.
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
from vrenderer_pathtracer_amd.renderer import SURF_MESH, SURF_NONE  # noqa: E402


def camera_rays(r, n):
    """The first n pixels' camera rays, row-major, wrapped."""
    o, d = r.cameraRays()
    i = torch.arange(n, device=o.device) % o.shape[0]
    return o[i].contiguous(), d[i].contiguous()


def random_rays(lo, hi, n, dev, seed=7):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    o = torch.rand((n, 3), generator=g, device=dev) * (hi - lo)[None, :] + lo[None, :]
    d = torch.randn((n, 3), generator=g, device=dev)
    return o.contiguous(), (d / d.norm(dim=1, keepdim=True)).contiguous()


def time_call(call, stream, warm=2, reps=5):
    torch.cuda.synchronize()
    ms = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = call()
        e1.record(stream)
        e1.synchronize()
        assert rc == 0, rc
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    return ms


def measure(cfg, n_rays):
    dev = torch.device("cuda", 0)
    sc = scenes.make_scene(cfg)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    stream = torch.cuda.ExternalStream(r.get_stream(), device=dev)
    verts = torch.from_numpy(np.ascontiguousarray(sc["mesh_flat"]["verts"][:, :3])).to(dev)
    out = {"scene": cfg, "n_slots": int(verts.shape[0]), "depth": r.bvh_info()[0], "walk": "culled", "n_rays": n_rays,
           "resolution": [sc["width"], sc["height"]]}
    sets = {"camera": camera_rays(r, n_rays),
            "random": random_rays(verts.min(0).values, verts.max(0).values, n_rays, dev)}
    p = lambda t: ctypes.c_void_p(t.data_ptr())                             # noqa: E731
    L, ctx = r._lib, r._ctx
    for name, (o, d) in sets.items():
        seeds = torch.randint(-2**31, 2**31, (n_rays, 2), dtype=torch.int32, device=dev)
        surf = torch.empty((n_rays, 28), dtype=torch.float32, device=dev)
        rad = torch.empty((n_rays, 4), dtype=torch.float32, device=dev)
        hit = torch.empty((n_rays, 4), dtype=torch.int32, device=dev)
        calls = {"surface": lambda: L.vrhip_trace_surface(ctx, p(o), p(d), n_rays, p(surf)),
                 "radiance1": lambda: L.vrhip_trace_radiance(ctx, p(o), p(d), p(seeds), n_rays, 1, p(rad)),
                 "closest": lambda: L.vrhip_trace_rays(ctx, p(o), p(d), None, n_rays, 0, p(hit))}
        for what, call in calls.items():
            ms = time_call(call, stream)
            out[f"{name}_{what}_mrays_s"] = round(n_rays / min(ms) / 1e3, 1)
            out[f"{name}_{what}_ms_all"] = [round(m, 4) for m in ms]
        kind = surf.view(torch.int32)[:, 1]
        out[f"{name}_hit_share"] = round(float((kind != SURF_NONE).float().mean()), 4)
        out[f"{name}_mesh_share"] = round(float((kind == SURF_MESH).float().mean()), 4)
        out[f"{name}_surface_over_radiance1"] = round(out[f"{name}_surface_mrays_s"] / out[f"{name}_radiance1_mrays_s"], 3)
    r.cleanUp()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--rays", type=int, default=1 << 20)
    a = ap.parse_args()
    lines = []
    for cfg in ("C2", "C5"):
        lines.append(json.dumps(measure(cfg, a.rays)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
