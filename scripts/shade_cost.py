#!/usr/bin/env python3
"""Rate of the surface-record radiance kernel (VRendererHIP.shadeSurface,
vrhip_shade_surface) beside the radiance query's on the same rays, culled walk.

  python scripts/shade_cost.py [--out profiles/shade/cost.json] [--rays 1048576]
                               [--scenes C2,C5] [--label head]

One JSON line per scene (C2: Cornell box + the 10k-triangle knot; C5: HDRI +
the 1M-triangle knot, both with the host-built tree the scene loads).  The
records are traceSurface's along the two ray sets of scripts/radiance_cost.py:
  camera   the scene camera's rays at the scene's resolution, pixel after
           pixel in row-major order, repeated until --rays rays are filled
  random   origins uniform in the mesh's bounds, directions uniform on the sphere
and for 2 and for 32 paths per record:
  <set>_s<k>_shade_mpaths_s      records x paths over the best of 5 synchronous
  <set>_s<k>_radiance_mpaths_s   calls after 2 warm-up calls, each timed by
                                 events recorded on the context stream around
                                 the call, into a pre-allocated result buffer
  <set>_s<k>_ratio               shade over radiance
  *_ms_all                       the timed calls
The two calls alternate, shadeSurface then traceRadiance, warm-ups included, so
that both figures come from the same minutes.  The results are compared once
per set: shadeSurface's rgb must be traceRadiance's bit for bit.
--label names the library measured (the loader takes another build of the same
ABI from VRHIP_LIB), so that variant builds can be measured by one run each and
told apart in one file (profiles/shade/variants.json).  No bar is set for these
rates.
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from radiance_cost import camera_rays, random_rays  # noqa: E402
from vrenderer_pathtracer_amd import VRendererHIP, build_id, scenes  # noqa: E402

SAMPLES = (2, 32)


def time_both(r, rec, o, d, s, samples, stream, warm=2, reps=5):
    n = o.shape[0]
    out_s = torch.empty((n, 4), dtype=torch.float32, device=o.device)
    out_r = torch.empty((n, 4), dtype=torch.float32, device=o.device)
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr())                             # noqa: E731
    calls = (lambda: r._lib.vrhip_shade_surface(r._ctx, p(rec), p(d), p(s), n, samples, p(out_s)),
             lambda: r._lib.vrhip_trace_radiance(r._ctx, p(o), p(d), p(s), n, samples, p(out_r)))
    ms = ([], [])
    for i in range(warm + reps):
        for which, call in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = call()
            e1.record(stream)
            e1.synchronize()
            assert rc == 0, rc
            if i >= warm:
                ms[which].append(e0.elapsed_time(e1))
    a, b = out_s[:, :3].contiguous().view(torch.int32), out_r[:, :3].contiguous().view(torch.int32)
    return ms[0], ms[1], int((a != b).any(1).sum())


def measure(cfg, n_rays, label):
    dev = torch.device("cuda", 0)
    sc = scenes.make_scene(cfg)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    stream = torch.cuda.ExternalStream(r.get_stream(), device=dev)
    verts = torch.from_numpy(np.ascontiguousarray(sc["mesh_flat"]["verts"][:, :3])).to(dev)
    out = {"label": label, "scene": cfg, "n_slots": int(verts.shape[0]), "depth": r.bvh_info()[0], "walk": "culled",
           "n_records": n_rays, "resolution": [sc["width"], sc["height"]], "build_id": build_id()["build_id"]}
    sets = {"camera": camera_rays(r, sc, n_rays),
            "random": random_rays(verts.min(0).values, verts.max(0).values, n_rays, dev)}
    for name, (o, d, s) in sets.items():
        hits = r.traceSurface(o, d)
        rec = hits["record"]
        out[f"{name}_hit_fraction"] = round(float((hits["kind"] != 0).float().mean()), 4)
        for k in SAMPLES:
            ms_s, ms_r, differ = time_both(r, rec, o, d, s, k, stream)
            out[f"{name}_s{k}_shade_mpaths_s"] = round(n_rays * k / min(ms_s) / 1e3, 1)
            out[f"{name}_s{k}_radiance_mpaths_s"] = round(n_rays * k / min(ms_r) / 1e3, 1)
            out[f"{name}_s{k}_ratio"] = round(min(ms_r) / min(ms_s), 4)
            out[f"{name}_s{k}_shade_ms_all"] = [round(m, 4) for m in ms_s]
            out[f"{name}_s{k}_radiance_ms_all"] = [round(m, 4) for m in ms_r]
            out[f"{name}_s{k}_records_differing"] = differ
    r.cleanUp()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--scenes", default="C2,C5")
    ap.add_argument("--label", default="head", help="names the library measured (VRHIP_LIB)")
    a = ap.parse_args()
    lines = []
    for cfg in a.scenes.split(","):
        lines.append(json.dumps(measure(cfg, a.rays, a.label)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
