"""The SAH cost of a flattened tree on the host (vrhip_flat_sah_cost), the
yardstick for the device value of vrhip_bvh_sah_cost, and the refit entry
points' refusals that need no device."""
import ctypes
import math

import numpy as np
import pytest

from vrenderer_pathtracer_amd import _native, build_flat, flat_sah_cost, scenes

TERM = 0x80000000


def numpy_sah_cost(flat):
    """(sum over inner nodes of area(own box) + sum over leaves of area(leaf
    box) x triangle count) / area(root box), area = dx dy + dy dz + dz dx in
    fp64 from the fp32 boxes; every node reachable from the root, once."""
    nodes = np.asarray(flat["bvh"], np.float32).reshape(-1, 4, 4)
    child = nodes[:, 3, :2].copy().view(np.int32)
    is_term = np.asarray(flat["verts"], np.float32)[:, 0].copy().view(np.uint32) == TERM
    term_pos = np.flatnonzero(is_term)
    n64 = nodes.astype(np.float64)
    # child boxes: [c0 lo.x hi.x lo.y hi.y] [c1 ...] [c0 lo.z hi.z c1 lo.z hi.z]
    lo = np.stack([np.stack([n64[:, c, 0], n64[:, c, 2], n64[:, 2, 2 * c]], -1) for c in range(2)], 1)   # (N, 2, 3)
    hi = np.stack([np.stack([n64[:, c, 1], n64[:, c, 3], n64[:, 2, 2 * c + 1]], -1) for c in range(2)], 1)

    def area(lo, hi):
        d = hi - lo
        return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]

    own = area(lo.min(1), hi.max(1))
    child_area = area(lo, hi)
    total, seen, stack = 0.0, set(), [0]
    terms = 0
    while stack:
        n = stack.pop()
        assert n not in seen
        seen.add(n)
        total += own[n]
        terms += 1
        for c in range(2):
            idx = int(child[n, c])
            if idx >= 0:
                stack.append(idx // 4)
                continue
            start = ~idx
            count = (term_pos[np.searchsorted(term_pos, start)] - start) // 3
            total += child_area[n, c] * count
            terms += 1
    assert terms < 10 ** 4                           # the tolerance below is argued for fewer terms than this
    return total / own[0] if 0 < own[0] < math.inf else math.inf


def two_triangles():
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 7, 9]], np.float32)
    return dict(positions=P, normals=np.zeros_like(P), tangents=np.zeros_like(P), uvs=np.zeros((6, 2), np.float32),
                tris=np.arange(6, dtype=np.uint32).reshape(-1, 3))


def flat_soup(n, seed):
    """test_gpu_device_build.soup(n, seed) with z = 0 everywhere (its flat_axis mesh)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-30.0, 30.0, (n, 1, 3))
    P = (c + rng.normal(0, 4.0, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    P[:, 2] = 0.0
    return dict(positions=P, normals=np.zeros_like(P), tangents=np.zeros_like(P),
                uvs=np.zeros((3 * n, 2), np.float32), tris=np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))


# All terms are positive and fewer than 10^4, so the error of summing them in
# another order is below 10^4 * 2^-53 ~ 1e-12 relative; 1e-9 leaves three decades.
REL = 1e-9


@pytest.mark.parametrize("name", ["knot", "two_triangles", "flat_axis"])
def test_flat_sah_cost_equals_numpy(native, name):
    mesh = {"knot": lambda: scenes.torus_knot(40, 20), "two_triangles": two_triangles,
            "flat_axis": lambda: flat_soup(80, 6)}[name]()
    flat = build_flat(mesh)
    want = numpy_sah_cost(flat)
    got = flat_sah_cost(flat)
    print(name, "flat_sah_cost", got, "numpy", want)
    assert math.isfinite(want) and want > 0
    assert abs(got - want) <= REL * want
    if name == "flat_axis":
        # z = 0: every box is degenerate along z, its area is exactly dx * dy
        nodes = flat["bvh"].reshape(-1, 4, 4)
        assert (nodes[:, 2, :] == 0).all()
        lo = np.minimum(nodes[0, 0, [0, 2]], nodes[0, 1, [0, 2]]).astype(np.float64)
        hi = np.maximum(nodes[0, 0, [1, 3]], nodes[0, 1, [1, 3]]).astype(np.float64)
        assert (hi - lo).prod() > 0                  # the root's area


def test_one_point_mesh_costs_infinity(native):
    P = np.tile(np.array([[1.5, -2.0, 3.0]], np.float32), (6, 1))
    flat = build_flat(dict(two_triangles(), positions=P))
    assert flat_sah_cost(flat) == math.inf           # status OK: no exception


def test_corrupted_tree_is_err_bvh(native):
    flat = build_flat(scenes.torus_knot(20, 10))
    corruptions = []
    bad = {k: v.copy() for k, v in flat.items()}
    bad["bvh"][3, 0] = np.array([10 ** 6], np.int32).view(np.float32)[0]        # child out of range
    corruptions.append(bad)
    bad = {k: v.copy() for k, v in flat.items()}
    bad["bvh"][3, 0] = np.array([0], np.int32).view(np.float32)[0]              # cycle back to the root
    corruptions.append(bad)
    bad = {k: v.copy() for k, v in flat.items()}
    term = np.where(bad["verts"][:, 0].view(np.uint32) == TERM)[0]
    bad["verts"][term[-1], 0] = 1.0                                              # lost terminator
    corruptions.append(bad)
    for bad in corruptions:
        with pytest.raises(_native.VRHIPError) as e:
            flat_sah_cost(bad)
        assert e.value.code == -4                    # VRHIP_ERR_BVH
    assert math.isfinite(flat_sah_cost(flat))


def test_null_context_is_invalid_without_a_device(native):
    cost = ctypes.c_double(-1.0)
    assert native.vrhip_refit_mesh_device(None, None, None, None, 3) == -1
    assert native.vrhip_refit_mesh_device(None, ctypes.c_void_p(256), None, None, 3) == -1
    assert native.vrhip_bvh_sah_cost(None, ctypes.byref(cost)) == -1
    assert cost.value == -1.0
