#!/usr/bin/env python3
"""Cost of the lightmap atlas call (VRendererHIP.atlasRecords,
vrhip_atlas_surface).

  python scripts/atlas_cost.py [--out profiles/atlas/cost.json]

One JSON line per mesh (the 10k-triangle and the 1M-triangle unwrapped knot,
scenes.torus_knot_unwrapped(100, 50) and (1000, 500) with margin 0.02, built on
the device with the Morton builder, under the HDRI with the three maps loaded)
with, for each atlas size (1024^2, 4096^2) and gutter (0, 4):
  atlas_<side>_g<gutter>_ms       ms per synchronous call, best of 5 after 2
                                  warm-up calls, timed by events on the context
                                  stream, into a pre-allocated record buffer
  atlas_<side>_g<gutter>_ms_all   the timed calls
  store_floor_<side>_ms           the time the records alone need at the
                                  device's write rate: 112 B per texel over
                                  --hbm-gbs (default 8000 GB/s, the MI355X's
                                  HBM3E peak)
  surface_<side>_ms               vrhip_trace_surface on as many camera rays
                                  (the scene camera's rays, repeated) in the
                                  same process: the other producer of records
  covered_<side>                  the share of texels that hold a record, gutter 0
No bar is set for these times: nothing exists to compare them with.
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
from vrenderer_pathtracer_amd.renderer import SURF_MESH  # noqa: E402

SIDES = (1024, 4096)
GUTTERS = (0, 4)


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


def measure(nu, nv, hbm_gbs):
    dev = torch.device("cuda", 0)
    sc = scenes.make_scene("C3", 1280, 720)
    sc["mesh_flat"] = None
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    mesh = scenes.torus_knot_unwrapped(nu, nv, 0.02)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)      # noqa: E731
    r.initMeshDevice(t(mesh["positions"], np.float32), t(mesh["tris"], np.int32), t(mesh["normals"], np.float32),
                     t(mesh["tangents"], np.float32), t(mesh["uvs"], np.float32), max_leaf_tris=2 if nu * nv <= 50000 else 4)
    stream = torch.cuda.ExternalStream(r.get_stream(), device=dev)
    out = {"mesh": f"unwrapped knot {nu}x{nv}", "triangles": int(len(mesh["tris"])), "builder": "morton",
           "depth": r.bvh_info()[0], "hbm_gbs": hbm_gbs}
    p = lambda x: ctypes.c_void_p(x.data_ptr())                                 # noqa: E731
    L, ctx = r._lib, r._ctx
    o, d = r.cameraRays()
    for side in SIDES:
        n = side * side
        rec = torch.empty((n, 28), dtype=torch.float32, device=dev)
        for g in GUTTERS:
            ms = time_call(lambda: L.vrhip_atlas_surface(ctx, side, side, g, p(rec)), stream)
            out[f"atlas_{side}_g{g}_ms"] = round(min(ms), 4)
            out[f"atlas_{side}_g{g}_ms_all"] = [round(m, 4) for m in ms]
            if g == 0:
                out[f"covered_{side}"] = round(float((rec.view(torch.int32)[:, 1] == SURF_MESH).float().mean()), 4)
        out[f"store_floor_{side}_ms"] = round(112.0 * n / (hbm_gbs * 1e9) * 1e3, 4)
        i = torch.arange(n, device=dev) % o.shape[0]
        oo, dd = o[i].contiguous(), d[i].contiguous()
        ms = time_call(lambda: L.vrhip_trace_surface(ctx, p(oo), p(dd), n, p(rec)), stream)
        out[f"surface_{side}_ms"] = round(min(ms), 4)
        out[f"surface_{side}_ms_all"] = [round(m, 4) for m in ms]
        del rec, oo, dd
    r.cleanUp()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    a = ap.parse_args()
    lines = []
    for nu, nv in ((100, 50), (1000, 500)):
        lines.append(json.dumps(measure(nu, nv, a.hbm_gbs)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
