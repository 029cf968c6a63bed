#!/usr/bin/env python3
"""Cost of the probe query (VRendererHIP.probeSH, vrhip_probe_sh) against the
composition it replaces.

  python scripts/probe_cost.py [--out profiles/probe/cost.json] [--reps 5]

The comparator is what a caller does without the call: expand the
n_probes x n_dirs rays and their seeds in torch, traceRadiance on them, and
project with a torch fp32 einsum against the weighted basis.  Both run in one
process on the same inputs, alternating, `--reps` timed repeats each after two
warm-up rounds; every call is synchronous (wall clock around the call, the
comparator closed by torch.cuda.synchronize()).

One JSON line per (scene, workload, direction order):
  scene          C2 (Cornell box, spheres) or C5 (the knot under the HDRI)
  probes, dirs   a 16x16x8 grid with 256 and with 1,024 directions, and
                 32,768 probes (32x32x32) with 64; 2 paths per ray
  compact        scenes.probe_directions(k, compact): blocks of 64 that are
                 caps of the sphere, or the plain Fibonacci order
  fused_ms, composed_ms         median of the repeats; *_all the repeats
  fused_mpaths, composed_mpaths probes * dirs * samples / median time
  composed_spread               (max - min) / median of the comparator's repeats
  fused_torch_peak, composed_torch_peak   torch.cuda.max_memory_allocated over
                 a call, above what was allocated before it (inputs excluded)
  fused_scratch  the library's own scratch for the call (vr_probe.hpp
                 probe_scratch_bytes: n_probes * ceil(n_dirs / 64) * 112 bytes
                 with more than one block, else 0), outside torch's allocator
  max_abs_diff   largest |fused - composed| coefficient (the einsum's order of
                 summation is not pinned; the fused call's is)
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrenderer_pathtracer_amd import VRendererHIP, scenes  # noqa: E402

SAMPLES = 2
BOXES = {"C2": ((-40.0, 40.0), (-40.0, 40.0), (-80.0, 40.0)), "C5": ((-40.0, 40.0),) * 3}
WORKLOADS = (((16, 16, 8), 256), ((16, 16, 8), 1024), ((32, 32, 32), 64))


def grid(shape, box, dev):
    axes = [torch.linspace(lo, hi, n, dtype=torch.float64) for n, (lo, hi) in zip(shape, box)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).float().contiguous().to(dev)


def weighted_basis(d, w):
    """[K, 9]: w_k * Y_j(d_k) in fp32, as a caller would write it."""
    u = d / d.norm(dim=-1, keepdim=True)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    Y = torch.stack([torch.full_like(x, 0.282094792), 0.488602512 * y, 0.488602512 * z, 0.488602512 * x,
                     1.09254843 * x * y, 1.09254843 * y * z, 0.315391565 * (3.0 * z * z - 1.0), 1.09254843 * x * z,
                     0.546274215 * (x * x - y * y)], -1)
    return (w[:, None] * Y).contiguous()


def composed(r, pts, d, w, ps, ds):
    n, k = pts.shape[0], d.shape[0]
    o = pts.repeat_interleave(k, 0)
    dd = d.repeat(n, 1)
    s = (ps[:, None, :] ^ ds[None, :, :]).reshape(-1, 2).contiguous()
    rec = r.traceRadiance(o, dd, s, samples=SAMPLES)
    sh = torch.einsum("pkc,kj->pjc", rec.view(n, k, 4)[:, :, :3], weighted_basis(d, w))
    torch.cuda.synchronize()
    return sh


def fused(r, pts, d, w, ps, ds):
    return r.probeSH(pts, d, w, ps, ds, samples=SAMPLES)


def peak_of(fn, *a):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(*a)
    torch.cuda.synchronize()
    return out, int(torch.cuda.max_memory_allocated() - base)


def measure(cfg, reps):
    dev = torch.device("cuda", 0)
    r = VRendererHIP(0)
    scenes.load_into(r, scenes.make_scene(cfg))
    lines = []
    for shape, k in WORKLOADS:
        pts = grid(shape, BOXES[cfg], dev)
        n = pts.shape[0]
        g = torch.Generator(device=dev).manual_seed(1)
        ps = torch.randint(-2**31, 2**31, (n, 2), dtype=torch.int32, device=dev, generator=g)
        ds = torch.randint(-2**31, 2**31, (k, 2), dtype=torch.int32, device=dev, generator=g)
        for compact in (True, False):
            dn, wn = scenes.probe_directions(k, compact)
            d, w = torch.from_numpy(dn).to(dev), torch.from_numpy(wn).to(dev)
            a = (r, pts, d, w, ps, ds)
            f, f_peak = peak_of(fused, *a)
            c, c_peak = peak_of(composed, *a)
            diff = float((f[:, :27].view(n, 9, 3) - c).abs().max())
            del f, c
            tf, tc = [], []
            for i in range(2 + reps):
                for fn, ts in ((fused, tf), (composed, tc)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(*a)
                    ts.append((time.perf_counter() - t0) * 1e3)
            tf, tc = tf[2:], tc[2:]
            mf, mc = float(np.median(tf)), float(np.median(tc))
            paths = n * k * SAMPLES
            nb = -(-k // 64)
            lines.append(dict(scene=cfg, probes=n, dirs=k, samples=SAMPLES, compact=compact,
                              fused_ms=round(mf, 3), composed_ms=round(mc, 3),
                              fused_ms_all=[round(t, 3) for t in tf], composed_ms_all=[round(t, 3) for t in tc],
                              fused_mpaths=round(paths / mf / 1e3, 1), composed_mpaths=round(paths / mc / 1e3, 1),
                              composed_spread=round((max(tc) - min(tc)) / mc, 4),
                              fused_torch_peak=f_peak, composed_torch_peak=c_peak,
                              fused_scratch=n * nb * 112 if nb > 1 else 0, max_abs_diff=diff))
            print(json.dumps(lines[-1]), flush=True)
    r.cleanUp()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="C2,C5")
    a = ap.parse_args()
    lines = []
    for cfg in a.scenes.split(","):
        lines += measure(cfg, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
