#!/usr/bin/env python3
"""Cost of the denoiser (VRendererHIP.denoise, vrhip_denoise).

  python scripts/denoise_cost.py [--out profiles/denoise/cost.json] [--label lds]

One JSON line per resolution (1280 x 720 and 3840 x 2160) for the library that
is loaded (VRHIP_LIB picks a build variant; --label names it in the line).
Inputs: scene C2 at that resolution, one rendered frame as the colour and the
surface query on the camera's rays as the guides, so every cell is valid and
every tap is evaluated.  Timed are synchronous calls of vrhip_denoise with the
default parameters into a pre-allocated output, by events recorded on the
context stream around each call: 5 warm-up calls, then 30, reported as median,
minimum, maximum and all.  The calls with 0 to 5 passes are timed the same way;
pass_ms[j] is the difference of the medians of j + 1 and j passes.
Beside each time stands the traffic floor: per pass 3 float4 planes read and 1
written per cell, prep 4 of the record's 7 rows and the colour read and 3
planes written, final 1 plane and 1 record row read and 1 plane written, at the
HBM rate given by --tbs (terabytes per second; the default is 8.0, the MI355X's
nominal rate).  At 1280 x 720 the four planes are 59 MB and stay in the 256 MB
last-level cache between the launches, so that figure is a floor for HBM
traffic only, not for the call.  No bar is set for these times.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]

import torch  # noqa: E402

from vrenderer_pathtracer_amd import VRendererHIP, _native, scenes  # noqa: E402


def time_call(call, stream, warm=5, reps=30):
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


def floor_bytes(n, passes):
    prep = n * (4 * 16 + 16 + 3 * 16)
    final = n * (16 + 16 + 16)
    return prep + final + passes * n * 4 * 16


def measure(w, h, label, tbs):
    dev = torch.device("cuda", 0)
    sc = scenes.make_scene("C2", w, h)
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    r.render(frames=1, times=[sc["time"]])
    stream = torch.cuda.ExternalStream(r.get_stream(), device=dev)
    color = torch.from_numpy(r.read_accum()).to(dev).contiguous()
    o, d = r.cameraRays()
    guides = r.traceSurface(o, d)["record"]
    out = torch.empty_like(color)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                             # noqa: E731
    dflt = VRendererHIP.DENOISE_DEFAULTS
    n = w * h
    line = {"label": label, "lib": _native.build_id()["lib"], "resolution": [w, h], "scene": "C2",
            "valid_share": round(float((guides.view(torch.int32)[:, 1] > 0).float().mean()), 4), "params": dflt}
    med = []
    for passes in range(6):
        prm = _native.DenoiseParams(passes, 1, dflt["normal_power_log2"], dflt["sigma_color"], dflt["sigma_position"])
        ms = time_call(lambda: r._lib.vrhip_denoise(r._ctx, p(color), p(guides), w, h, ctypes.byref(prm), p(out)), stream)
        med.append(statistics.median(ms))
        if passes == dflt["passes"]:
            line.update(ms_median=round(med[-1], 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                        ms_all=[round(m, 4) for m in ms])
    line["ms_median_by_passes"] = [round(m, 4) for m in med]
    line["pass_ms"] = [round(med[j + 1] - med[j], 4) for j in range(5)]
    line["floor_bytes"] = floor_bytes(n, dflt["passes"])
    line["floor_tb_s"] = tbs
    line["floor_ms"] = round(line["floor_bytes"] / (tbs * 1e12) * 1e3, 4)
    line["pass_floor_ms"] = round(n * 64 / (tbs * 1e12) * 1e3, 4)
    r.cleanUp()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the lines to this file")
    ap.add_argument("--label", default="shipped")
    ap.add_argument("--tbs", type=float, default=8.0)
    a = ap.parse_args()
    lines = []
    for w, h in ((1280, 720), (3840, 2160)):
        lines.append(json.dumps(measure(w, h, a.label, a.tbs)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
