"""The host builder, the SAH cost and the host ray walk at the extremes of
float (tests/extreme_cases.py), without a device.  The host walk is the
yardstick of the device query (test_gpu_extreme.py), so it is pinned here
against numpy: the reference's span restated with its NaN and signed-zero
behaviour (ray_query_cases._span), the triangle test spelt out in float32, the
first of the closest over the pierced leaves.  At these magnitudes the brute
force over all triangles is no expectation any more: slab arithmetic that
overflows makes the reference's walk miss triangles its own triangle test
accepts, and the non-vacuity test counts them."""
import functools
import math

import numpy as np
import pytest

import extreme_cases as ec
from device_mesh_cases import hard_mesh, soup
from extreme_cases import EXTREME_KINDS, assert_same_records, check_boxes_and_leaves, extreme_mesh, extreme_ray_set
from ray_query_cases import flat_triangles, same_bits, u32
from test_refit_cpu import numpy_sah_cost
from vrenderer_pathtracer_amd import build_flat, flat_sah_cost, flat_trace_rays, validate_flat

N_RAYS = 2048
WALK_MESHES = {"soup200": lambda: soup(200), "big": lambda: extreme_mesh("big"), "far": lambda: hard_mesh("far")}


@functools.lru_cache(maxsize=None)
def host_tree(kind, leaf):
    mesh = extreme_mesh(kind)
    return mesh, build_flat(mesh, max_leaf_tris=leaf)


@functools.lru_cache(maxsize=None)
def walk_case(name):
    """(flat, rays, host records, numpy records, brute-force hit): computed once, never written."""
    flat = build_flat(WALK_MESHES[name](), 2)
    _, V = flat_triangles(flat)
    rays = extreme_ray_set(V, N_RAYS)
    got = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"])
    want, brute_hit = ec.walk_expectation(flat, rays)
    return flat, rays, got, want, brute_hit


# ---- 1. the host builder ----------------------------------------------------------------
@pytest.mark.parametrize("leaf", [1, 3])
@pytest.mark.parametrize("kind", EXTREME_KINDS)
def test_host_builder_at_the_extremes(native, kind, leaf):
    """A valid tree, every input triangle in exactly one leaf, every stored box
    the exact fp32 min/max of what lies beneath it."""
    mesh, flat = host_tree(kind, leaf)
    depth, n_nodes = check_boxes_and_leaves(flat, mesh, leaf)
    assert (depth, n_nodes) == validate_flat(flat)
    assert np.isfinite(flat["bvh"].reshape(-1, 4, 4)[:, :3]).all()


def test_the_meshes_reach_what_they_are_for(native):
    big, huge, tiny = (extreme_mesh(k)["positions"] for k in ("big", "huge", "tiny"))
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(big.max()) * np.float32(big.max()))            # a product of two coordinates
        assert np.isinf(huge.max(0) - huge.min(0)).all()                             # the extent on every axis
        V = huge.reshape(-1, 3, 3)
        centroid = np.float32(0.5) * (V.min(1) + V.max(1))                           # the builder's 0.5f * (lo + hi)
        assert np.isinf(centroid).any() and not np.isnan(centroid).any()
    assert (np.abs(tiny[tiny != 0]) < np.finfo(np.float32).tiny).all()               # every coordinate denormal


def test_wide_builds_next_to_the_depth_cap(native):
    """WIDE_SEED is a seed whose tree the host builds with leaves of 1 and of 3:
    29 levels of inner nodes under a cap of 30, leaves at the cap above max_leaf."""
    for leaf in (1, 3):
        mesh, flat = host_tree("wide", leaf)
        depth, _ = validate_flat(flat)
        assert depth == ec.MAX_BUILD_DEPTH - 1


# ---- 2. the SAH cost ----------------------------------------------------------------------
# As tests/test_refit_cpu.py: fewer than 10^4 positive fp64 terms in another order.
REL = 1e-9


@pytest.mark.parametrize("leaf", [1, 3])
@pytest.mark.parametrize("kind", EXTREME_KINDS)
def test_flat_sah_cost_at_the_extremes(native, kind, leaf):
    """Equal to the numpy sum, and +infinity where vrhip.h says so: a root area
    that is 0 or not finite.  fp64 holds every area of big, wide and tiny
    (at most (7e38)^2 x 3); huge's root is 6.8e38 wide and its area finite too."""
    _, flat = host_tree(kind, leaf)
    want, got = numpy_sah_cost(flat), flat_sah_cost(flat)
    print(kind, leaf, "flat_sah_cost", got, "numpy", want)
    assert not math.isnan(got)
    if math.isinf(want):
        assert got == math.inf
    else:
        assert want > 0 and abs(got - want) <= REL * want


def test_flat_sah_cost_is_infinite_for_a_root_without_area(native):
    """All 200 triangles on one denormal point: the root's area is 0."""
    m = extreme_mesh("tiny")
    m["positions"][:] = m["positions"][0]
    flat = build_flat(m, 3)
    assert numpy_sah_cost(flat) == math.inf and flat_sah_cost(flat) == math.inf


# ---- 3. the host walk against numpy ------------------------------------------------------------
@pytest.mark.parametrize("name", list(WALK_MESHES))
def test_host_walk_equals_the_numpy_walk(native, name):
    flat, rays, got, want, _ = walk_case(name)
    assert_same_records(got, want, f"{name}: host walk against numpy")
    miss = got["prim"] < 0
    assert same_bits(got["t"][miss], rays["tmax"][miss])                 # a miss returns its tmax bits
    assert not u32(got["u"][miss]).any() and not u32(got["v"][miss]).any()
    assert not np.isnan(got["t"]).any()
    # any-hit: the same rays hit, the records are {0,0,0,0} or the miss record
    anyh = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"], any_hit=True)
    assert ((anyh["prim"] >= 0) == ~miss).all()
    assert not any(u32(anyh[k][~miss]).any() for k in ("t", "u", "v")) and not anyh["prim"][~miss].any()
    assert same_bits(anyh["t"][miss], rays["tmax"][miss])
    # without tmax the closest so far starts at 1e20
    open_got = flat_trace_rays(flat, rays["origins"][:512], rays["dirs"][:512])
    open_want, _ = ec.walk_expectation(flat, {k: v[:512] for k, v in rays.items()}, use_tmax=False)
    assert_same_records(open_got, open_want, f"{name}: without tmax")


def test_the_extreme_rays_are_not_vacuous(native):
    """On the ordinary 200-soup: hits, hit records with a NaN barycentric (the
    reference's `u < 0 || u > 1` lets a NaN through while dist stays finite),
    and rays the brute force over all triangles accepts and the walk misses."""
    _, rays, got, _, brute_hit = walk_case("soup200")
    hit = got["prim"] >= 0
    nan_bary = hit & (np.isnan(got["u"]) | np.isnan(got["v"]))
    lost = brute_hit & ~hit
    print("hits", hit.sum(), "with a NaN barycentric", nan_bary.sum(), "brute force only", lost.sum())
    assert hit.sum() >= 100 and nan_bary.sum() >= 10 and lost.sum() >= 30
    assert np.isfinite(got["t"][nan_bary]).all()
    assert set(rays["kind"]) == set(ec.DIR_KINDS)


@pytest.mark.parametrize("both", [True, False])
def test_nan_slabs_on_the_host_are_the_devices(native, both):
    """inf - inf on both planes of an axis hides every box, whatever the NaN's
    sign.  On one plane only (a box that straddles 0, the other plane -inf)
    the sign decides: set, as the device (and x86) makes it, and the box is
    missed; clear, and z would drop out of the span and the ray hit.  The
    numpy walk sets the sign explicitly (ray_query_cases.DEVICE_NAN), so the
    host walk must give the device's answer on any host."""
    mesh, rays = ec.nan_plane_case(both)
    flat = build_flat(mesh, 2)
    got = flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"])
    want, brute_hit = ec.walk_expectation(flat, rays)
    assert_same_records(got, want, f"both={both}")
    assert brute_hit.all()
    assert not (got["prim"] >= 0).any()
