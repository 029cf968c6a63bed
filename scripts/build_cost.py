#!/usr/bin/env python3
"""Cost of getting a mesh into the renderer: the BVH built on the device from
device-resident triangles (initMeshDevice, its Morton and its SAH builder)
against the host path (build_flat, then initMesh), and what each tree costs at
render time.

  python scripts/build_cost.py [--out build_cost.json] [--frames 16] [--steps 4]

One JSON line per mesh (the 10k-triangle knot in scene C2, the 1M-triangle knot
in scene C5):
  device_build_ms, sah_build_ms   median of 5 builds into fresh contexts after
                    one warm-up, wall clock around the synchronous call (the
                    Morton and the SAH builder)
  sah_build_vs_host   sah_build_ms over the host path (build_flat + initMesh)
  sah_arena_bytes, sah_arena_bytes_per_tri   the SAH build's device scratch
  host_build_flat_ms, host_init_mesh_ms   the host path in the same process
  depth_device, depth_sah, depth_host     as vrhip_bvh_info reports them
  mpaths_device_tree, mpaths_sah_tree, mpaths_host_tree    frames-per-step
                    render rate of the scene on each tree, measured as
                    scripts/ab.py does (median of 3 batches of back-to-back
                    steps); sah_rate_vs_host and sah_rate_vs_morton are ratios
                    of rates from this run
  refit_ms          median of 5 refits (refitMeshDevice) of the SAH tree to the
                    deformed knot after one warm-up, same clock; refit_below_sah_build
                    is the one condition: below sah_build_ms of this run
  deformations      per twist k (deform below): bvh_sah_cost and the render rate
                    on (a) the SAH tree built on the undeformed knot and refit,
                    (b) a SAH tree and (c) a Morton tree rebuilt on the deformed
                    positions, and the rate ratios (a)/(b), (a)/(c)
--refit-out writes the refit keys of each line to a second file.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from device_mesh_cases import deform  # noqa: E402  (the twist of tests/test_gpu_refit.py)
from vrenderer_pathtracer_amd import VRendererHIP, _native, build_flat, scenes  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def render_rate(r, sc, frames, steps):
    r.render(frames=frames, time_seed=sc["time"])     # warm-up
    r.clearBuffer()
    ts = []
    for b in range(3):
        t0 = time.perf_counter()
        for i in range(steps):
            j = b * steps + i
            r.render(frames=frames, times=[sc["time"] + j * frames + k for k in range(frames)], sync=False)
        r.sync()
        ts.append((time.perf_counter() - t0) / steps)
    paths = (sc["width"] // 16) * 16 * (sc["height"] // 16) * 16 * 2 * frames
    return paths / median(ts) / 1e6


REFIT_KEYS = ("scene", "knot", "n_tris", "max_leaf_tris", "device_build_ms", "sah_build_ms", "refit_ms", "refit_ms_all",
              "refit_below_sah_build", "refit_vs_sah_build", "refit_vs_morton_build", "frames_per_step", "deformations")


def measure(cfg, nu, nv, leaf, frames, steps):
    mesh = scenes.torus_knot(nu, nv)
    t0 = time.perf_counter()
    flat = build_flat(mesh, max_leaf_tris=leaf)
    host_build = time.perf_counter() - t0
    scenes._MESH_CACHE[(nu, nv, leaf)] = flat          # the scene below takes this tree instead of building it again
    sc = scenes.make_scene(cfg, knot=(nu, nv))
    assert sc["mesh_flat"] is flat

    r = VRendererHIP(0)
    r.init(sc["width"], sc["height"])
    t0 = time.perf_counter()
    r.initMesh(flat)
    host_init = time.perf_counter() - t0
    depth_host = r.bvh_info()[0]
    r.cleanUp()

    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(mesh[k])).to(dev) for k in ("positions", "normals", "tangents", "uvs")}
    d["tris"] = torch.from_numpy(np.ascontiguousarray(mesh["tris"], np.int32)).to(dev)
    torch.cuda.synchronize(dev)

    def device_build(r, builder="morton"):
        r.initMeshDevice(d["positions"], d["tris"], d["normals"], d["tangents"], d["uvs"], max_leaf_tris=leaf,
                         builder=builder)

    builds, depth_dev = {}, {}
    for builder in ("morton", "sah"):
        builds[builder] = []
        for i in range(6):                             # the first is the warm-up
            r = VRendererHIP(0)
            r.init(sc["width"], sc["height"])
            t0 = time.perf_counter()
            device_build(r, builder)
            builds[builder].append(time.perf_counter() - t0)
            depth_dev[builder] = r.bvh_info()[0]
            r.cleanUp()

    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    rate_host = render_rate(r, sc, frames, steps)
    r.cleanUp()
    rate = {}
    for builder in ("morton", "sah"):
        r = VRendererHIP(0)
        scenes.load_into(r, sc)
        device_build(r, builder)
        rate[builder] = render_rate(r, sc, frames, steps)
        r.cleanUp()
    # refit: the SAH tree built on the undeformed knot, moved to the deformed one
    moved = {k: torch.from_numpy(deform(mesh["positions"], k)).to(dev) for k in (0.03, 0.003)}
    torch.cuda.synchronize(dev)
    r = VRendererHIP(0)
    r.init(sc["width"], sc["height"])
    device_build(r, "sah")
    refits = []
    for i in range(6):                                 # the first is the warm-up
        t0 = time.perf_counter()
        r.refitMeshDevice(moved[0.03])
        refits.append(time.perf_counter() - t0)
    r.cleanUp()
    deformations = []
    for k, pos in moved.items():
        row = {"k": k}
        for key, builder, refit in (("refit_sah", "sah", True), ("rebuilt_sah", "sah", False),
                                    ("rebuilt_morton", "morton", False)):
            r = VRendererHIP(0)
            scenes.load_into(r, sc)
            if refit:
                device_build(r, builder)
                r.refitMeshDevice(pos)
            else:
                r.initMeshDevice(pos, d["tris"], d["normals"], d["tangents"], d["uvs"], max_leaf_tris=leaf,
                                 builder=builder)
            r.clearBuffer()
            row["sah_cost_" + key] = round(r.bvh_sah_cost(), 4)
            row["mpaths_" + key] = round(render_rate(r, sc, frames, steps), 1)
            r.cleanUp()
        row["refit_rate_vs_rebuilt_sah"] = round(row["mpaths_refit_sah"] / row["mpaths_rebuilt_sah"], 4)
        row["refit_rate_vs_rebuilt_morton"] = round(row["mpaths_refit_sah"] / row["mpaths_rebuilt_morton"], 4)
        deformations.append(row)
    refit_ms = median(refits[1:]) * 1e3
    n_tris = int(len(mesh["tris"]))
    arena = int(_native.lib().vrhip_device_sah_scratch_bytes(n_tris))
    sah_ms = median(builds["sah"][1:]) * 1e3
    return {"scene": cfg, "knot": [nu, nv], "n_tris": n_tris, "max_leaf_tris": leaf,
            "device_build_ms": round(median(builds["morton"][1:]) * 1e3, 3),
            "device_build_ms_all": [round(b * 1e3, 3) for b in builds["morton"][1:]],
            "sah_build_ms": round(sah_ms, 3), "sah_build_ms_all": [round(b * 1e3, 3) for b in builds["sah"][1:]],
            "host_build_flat_ms": round(host_build * 1e3, 3), "host_init_mesh_ms": round(host_init * 1e3, 3),
            "sah_build_vs_host": round(sah_ms / ((host_build + host_init) * 1e3), 5),
            "sah_arena_bytes": arena, "sah_arena_bytes_per_tri": round(arena / n_tris, 1),
            "depth_device": depth_dev["morton"], "depth_sah": depth_dev["sah"], "depth_host": depth_host,
            "frames_per_step": frames,
            "mpaths_device_tree": round(rate["morton"], 1), "mpaths_sah_tree": round(rate["sah"], 1),
            "mpaths_host_tree": round(rate_host, 1),
            "render_rate_ratio": round(rate["morton"] / rate_host, 4),
            "sah_rate_vs_host": round(rate["sah"] / rate_host, 4),
            "sah_rate_vs_morton": round(rate["sah"] / rate["morton"], 4),
            "refit_ms": round(refit_ms, 3), "refit_ms_all": [round(b * 1e3, 3) for b in refits[1:]],
            "refit_below_sah_build": bool(refit_ms < sah_ms), "refit_vs_sah_build": round(refit_ms / sah_ms, 4),
            "refit_vs_morton_build": round(refit_ms / (median(builds["morton"][1:]) * 1e3), 4),
            "deformations": deformations}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--refit-out", default=None, help="write the refit keys of each line to this file")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    lines, refit_lines = [], []
    for cfg, nu, nv, leaf in (("C2", 100, 50, 2), ("C5", 1000, 500, 4)):
        m = measure(cfg, nu, nv, leaf, a.frames, a.steps)
        lines.append(json.dumps(m))
        refit_lines.append(json.dumps({k: m[k] for k in REFIT_KEYS}))
        print(lines[-1], flush=True)
    if a.refit_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.refit_out)), exist_ok=True)
        with open(a.refit_out, "w") as f:
            f.write("\n".join(refit_lines) + "\n")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
