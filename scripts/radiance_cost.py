#!/usr/bin/env python3
"""Rate of the radiance query kernel (VRendererHIP.traceRadiance,
vrhip_trace_radiance), culled walk.

  python scripts/radiance_cost.py [--out profiles/radiance/cost.json] [--rays 1048576]
                                  [--bench C2=c2.json --bench C5=c5.json]

One JSON line per scene (C2: Cornell box + the 10k-triangle knot; C5: HDRI +
the 1M-triangle knot, both with the host-built tree the scene loads), with, for
2 and for 32 paths per ray:
  camera_s<k>_mpaths_s   the scene camera's rays at the scene's resolution
                         (cuda/src/PathTracer.cu:833-844, no jitter; the
                         un-normalised directions, as the call takes them),
                         pixel after pixel in row-major order, repeated from
                         the first pixel until --rays rays are filled
  random_s<k>_mpaths_s   origins uniform in the mesh's bounds, directions
                         uniform on the sphere
  *_ms_all               the timed calls
Each rate is rays x paths per ray over the best of 5 synchronous calls after 2
warm-up calls, timed by events recorded on the context stream around the
call, into a pre-allocated result buffer.
For context only, bench_mpaths_s: the `value` of a bench.py result line of the
same scene (--bench SCENE=file, a run of the same visit).  bench.py renders
whole frames through the path pool, whose lanes take a new path when theirs
ends; this kernel's lanes idle until their wave's slowest path has ended.  No
bar is set for these rates.
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

SAMPLES = (2, 32)


def camera_rays(r, sc, n):
    """The renderer's own camera rays (cameraRays(): the un-normalised directions, as the call takes them) and the
    seeds (x, y * time) render gives a pixel: the first n pixels, row-major, wrapped."""
    o, d = r.cameraRays()
    W = sc["width"]
    i = torch.arange(n, device=o.device) % o.shape[0]
    x, y = i % W, i // W
    seeds = torch.stack([x, (y * int(sc["time"])) & 0xFFFFFFFF], 1)
    seeds = torch.where(seeds >= 2**31, seeds - 2**32, seeds).to(torch.int32)
    return o[i].contiguous(), d[i].contiguous(), seeds.contiguous()


def random_rays(lo, hi, n, dev, seed=7):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    o = torch.rand((n, 3), generator=g, device=dev) * (hi - lo)[None, :] + lo[None, :]
    d = torch.randn((n, 3), generator=g, device=dev)
    s = torch.randint(-2**31, 2**31, (n, 2), generator=g, device=dev, dtype=torch.int32)
    return o.contiguous(), (d / d.norm(dim=1, keepdim=True)).contiguous(), s.contiguous()


def time_query(r, o, d, s, samples, stream, warm=2, reps=5):
    n = o.shape[0]
    out = torch.empty((n, 4), dtype=torch.float32, device=o.device)
    torch.cuda.synchronize()
    ms = []
    p = lambda t: ctypes.c_void_p(t.data_ptr())                             # noqa: E731
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = r._lib.vrhip_trace_radiance(r._ctx, p(o), p(d), p(s), n, samples, p(out))
        e1.record(stream)
        e1.synchronize()
        assert rc == 0, rc
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    return ms


def measure(cfg, n_rays, bench):
    dev = torch.device("cuda", 0)
    sc = scenes.make_scene(cfg)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    stream = torch.cuda.ExternalStream(r.get_stream(), device=dev)
    verts = torch.from_numpy(np.ascontiguousarray(sc["mesh_flat"]["verts"][:, :3])).to(dev)
    out = {"scene": cfg, "n_slots": int(verts.shape[0]), "depth": r.bvh_info()[0], "walk": "culled", "n_rays": n_rays,
           "resolution": [sc["width"], sc["height"]]}
    sets = {"camera": camera_rays(r, sc, n_rays),
            "random": random_rays(verts.min(0).values, verts.max(0).values, n_rays, dev)}
    for name, (o, d, s) in sets.items():
        for k in SAMPLES:
            ms = time_query(r, o, d, s, k, stream)
            out[f"{name}_s{k}_mpaths_s"] = round(n_rays * k / min(ms) / 1e3, 1)
            out[f"{name}_s{k}_ms_all"] = [round(m, 4) for m in ms]
    if cfg in bench:
        with open(bench[cfg]) as f:
            line = [json.loads(x) for x in f if x.startswith("{") and '"value"' in x][-1]
        out.update(bench_mpaths_s=line["value"], bench_metric=line.get("metric"), bench_verified=line.get("verified"))
    r.cleanUp()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--bench", action="append", default=[], metavar="SCENE=FILE",
                    help="a file holding bench.py's result line of that scene, from the same visit")
    a = ap.parse_args()
    bench = dict(b.split("=", 1) for b in a.bench)
    lines = []
    for cfg in ("C2", "C5"):
        lines.append(json.dumps(measure(cfg, a.rays, bench)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
