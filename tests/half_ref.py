"""The reference for the device BVH builder's outward fp32 -> fp16 box
rounding, and the values the tests check it on (shared by the host-only test
of vr::half_directed and the GPU test of vrhip_selftest_half_box)."""
import numpy as np


def half_reference(x, up):
    """np.float16(x), stepped one half ulp outward where it lies on the wrong
    side of x.  Reproduces half_bits_directed (vr_mesh_layout.cpp) on the values
    below: checked with a stand-alone host program that calls that function."""
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
        stepped = np.nextafter(h, np.float16(np.inf if up else -np.inf))
    wrong = (h.astype(np.float32) < x) if up else (h.astype(np.float32) > x)
    return np.where(wrong, stepped, h).astype(np.float16).view(np.uint16)


def half_values():
    rng = np.random.default_rng(17)
    sub = np.float32(2.0) ** -24
    v = [0.0, -0.0, sub, 3 * sub, 1023 * sub, 1023.5 * sub, sub / 2, sub / 3, 1e-10, 1e-30, 1e-45,
         65504.0, 65505.0, 65519.9, 65520.0, 1e6, 3e38]
    v += [2.0 ** e for e in range(-26, 18)]
    # the magnitudes of tests/extreme_cases.py: the first float past the largest half, the `huge` mesh, the largest float
    v += [np.nextafter(np.float32(65504.0), np.float32(np.inf)), 1e37, 3.4e38, np.finfo(np.float32).max]
    v = np.array(v, np.float32)
    bits = rng.integers(0, 0x7F800000, 10000, dtype=np.uint32)            # finite, then both signs
    bits |= rng.integers(0, 2, 10000, dtype=np.uint32) << np.uint32(31)
    return np.concatenate([v, -v, bits.view(np.float32)])
