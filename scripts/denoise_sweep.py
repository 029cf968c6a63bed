"""The sweep behind VRendererHIP.denoise's defaults (profiles/denoise/README.md).

CPU only: the filter is tests/denoise_driver.c, whose bits the kernels give,
on the two 64 x 48 oracle views of tests/denoise_cases.py (1 frame against the
mean of 256).  For every (sigma_color, sigma_position, normal_power_log2) at 5
passes with demodulation it prints RMSE(denoised, converged) /
RMSE(noisy, converged) per view and their geometric mean, sorted.

    python scripts/denoise_sweep.py
"""
import itertools
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import denoise_cases as dc  # noqa: E402

SIGMA_COLOR = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0)
SIGMA_POSITION = (0.125, 0.5, 2.0, 8.0, 32.0)
NORMAL_POWER_LOG2 = (1, 3, 5, 7)
PASSES = 5


def main():
    views = {name: dc.view(name) for name in dc.VIEW_NAMES}
    base = {name: dc.rmse(v[0], v[1]) for name, v in views.items()}
    rows = []
    for sc, sp, m in itertools.product(SIGMA_COLOR, SIGMA_POSITION, NORMAL_POWER_LOG2):
        ratios = []
        for name, (noisy, conv, rec) in views.items():
            out = dc.filtered(noisy, rec, dc.VIEW_W, dc.VIEW_H, PASSES, True, m, sc, sp)
            ratios.append(dc.rmse(out, conv) / base[name])
        rows.append((math.exp(sum(math.log(r) for r in ratios) / len(ratios)), sc, sp, m, ratios))
    rows.sort()
    print("RMSE(noisy, converged): " + ", ".join(f"{n} {b:.5f}" for n, b in base.items()))
    print(f"{'geo-mean':>8s} {'sigma_c':>8s} {'sigma_p':>8s} {'m':>2s}  " + "  ".join(dc.VIEW_NAMES))
    for g, sc, sp, m, ratios in rows:
        print(f"{g:8.4f} {sc:8.3f} {sp:8.3f} {m:2d}  " + "  ".join(f"{r:.4f}" for r in ratios))


if __name__ == "__main__":
    main()
