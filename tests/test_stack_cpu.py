"""The inputs of test_gpu_stack.py and their yardsticks, without a GPU: trees
that fill the traversal stack to its last entry (tests/stack_cases.py).

Shown here, for both kinds of tree at every depth the kernels' four stack
sizes turn on: the oracle's high-water mark equals the depth in every render
case of the GPU module; the rays of the query tests reach it too, wave by
wave, and are no single case repeated; the host walk agrees with a brute
force on them; and the yardstick would see a one-entry error: the oracle with
a stack of depth + 1 entries is the oracle, with one entry fewer (the push is
lost) at least a quarter of the pixels and of the rays' records change.  The
counts are printed (pytest -s) and recorded in profiles/stack/README.md."""
import numpy as np
import pytest

import pyoracle as po
import stack_cases as st
import surface_cases as sf
from ray_query_cases import brute_force, closest, dfs_slots, flat_triangles, same_bits, u32
from vrenderer_pathtracer_amd import flat_trace_rays
from vrenderer_pathtracer_amd.renderer import validate_flat

N_RAYS = 256
CASES = [(kind, depth) for kind in st.KINDS for depth in st.DEPTHS]
case = pytest.mark.parametrize("kind,depth", CASES, ids=[f"{k}-{d}" for k, d in CASES])


def _differ(a, b):
    """Pixels (or records) that differ in any byte."""
    a, b = (np.ascontiguousarray(x).view(np.uint8).reshape(-1, x.shape[-1] * x.itemsize) for x in (a, b))
    return int((a != b).any(-1).sum())


@case
def test_depth_is_the_argument(native, kind, depth):
    d, inner = validate_flat(st.tree(kind, depth))
    assert d == depth and inner == (depth if kind == "comb" else 2 * depth - 1)
    assert st.mesh_stack_entries(depth) == {15: 16, 16: 24, 23: 24, 24: 32, 30: 32, 31: 64, 62: 64}[depth]


def test_the_render_cases_are_the_issue_s():
    cases = st.render_cases()
    assert len(cases) == len(set(cases)) == 7 * 2 + 5 * 2 + 4 + 4 + 2
    assert {(k, d) for k, d, _ in cases} == {("comb", d) for d in st.DEPTHS} | {("legged", d) for d in st.LEGGED_DEPTHS}
    assert all(cfg in ("C2", "C3") or d <= 30 for _, d, cfg in cases)


@case
def test_filled_to_the_top(oracle, kind, depth):
    """max_stack == depth in every render case of the GPU module at this tree
    (and, for the legged comb, at the depths the GPU module leaves out), over
    two frames; every camera ray pierces every leaf box."""
    flat = st.tree(kind, depth)
    cfgs = [cfg for k, d, cfg in st.render_cases() if (k, d) == (kind, depth)] or ["C2", "C3"]
    for cfg in cfgs:
        sc = st.scene(flat, cfg)
        hx, hy = st.view_half_extent(sc, st.Z_FAR - 1.0)
        assert max(hx, hy) < st.VIEW
        cnt = st.oracle_render(sc, 2, count=True)[3]
        assert cnt["max_stack"] == depth, (cfg, cnt["max_stack"])
    for w, h in st.SMALL_IMAGES:
        assert st.oracle_render(st.scene(flat, "C2", w, h), 1, count=True)[3]["max_stack"] == depth


@case
def test_ray_marks(oracle, kind, depth):
    """high_water, the walk's push and pop rule restated, is the oracle's own
    count ray by ray; a quarter of the rays fill the stack, and every wave of
    64 holds a ray that does and one that stays below half."""
    flat, rays = st.tree(kind, depth), st.rays_of(kind, depth, N_RAYS)
    o, d = rays["origins"], sf.normalised(rays["dirs"])
    top = np.array([st.high_water(flat, o[i], d[i]) for i in range(N_RAYS)])
    _, counted = st.driver_rays(st.scene(flat, "C5"), o, rays["dirs"], 64)
    assert top.tolist() == counted.tolist()
    assert top.max() == depth and (top == depth).sum() >= N_RAYS / 4
    for w in range(0, N_RAYS, 64):
        assert (top[w:w + 64] == depth).any() and (top[w:w + 64] < depth / 2).any(), w
    print(f"\nhigh-water {kind}-{depth}: " + " ".join(f"{v}:{c}" for v, c in zip(*np.unique(top, return_counts=True))))


@case
def test_not_vacuous_and_walks_agree(native, kind, depth):
    """The host walk against the brute force over all triangles (a tie's
    winner is one of the closest, as in test_ray_query_cpu.py), with and
    without tmax; at least depth / 2 distinct triangles are a closest hit and
    some rays miss."""
    flat, rays = st.tree(kind, depth), st.rays_of(kind, depth, N_RAYS)
    slots, V = flat_triangles(flat)
    for tmax in (rays["tmax"], None):
        acc, dist, u, v = brute_force(V, rays["origins"], rays["dirs"], tmax)
        hit, tmin = closest(acc, dist)
        got = flat_trace_rays(flat, rays["origins"], rays["dirs"], tmax)
        assert (got["prim"] >= 0).tolist() == hit.tolist()
        assert same_bits(got["t"][hit], tmin[hit])
        col = np.searchsorted(slots, got["prim"][hit])
        assert (slots[col] == got["prim"][hit]).all()
        rows = np.flatnonzero(hit)
        assert acc[rows, col].all() and same_bits(dist[rows, col], tmin[hit])
        assert same_bits(got["u"][hit], u[rows, col]) and same_bits(got["v"][hit], v[rows, col])
        assert len(set(got["prim"][hit].tolist())) >= depth / 2
        assert 0 < (~hit).sum() < N_RAYS / 2
    below = np.array(st.TMAX_KINDS)[np.arange(N_RAYS) % 8] == "below"
    assert (flat_trace_rays(flat, rays["origins"], rays["dirs"], rays["tmax"])["prim"][below] == -1).all()


@case
def test_the_yardstick_sees_one_entry(oracle, kind, depth):
    """The oracle with a stack of a settable size (tests/stack_driver.c): with
    depth + 1 entries it is the oracle bit for bit, with depth entries, the
    last push lost, at least a quarter of the pixels and of the rays' records
    change.  A condition on the inputs, not a measurement."""
    flat, rays = st.tree(kind, depth), st.rays_of(kind, depth, N_RAYS)
    for cfg in ("C2", "C3"):
        sc = st.scene(flat, cfg)
        ref = st.oracle_render(sc, 2)
        exact = st.driver_render(sc, depth + 1, 2)
        assert [_differ(a, b) for a, b in zip(ref[:3], exact[:3])] == [0, 0, 0] and exact[3] == depth
        short = st.driver_render(sc, depth, 2)
        changed = _differ(ref[0], short[0])
        print(f"\nmutants {kind}-{depth} {cfg}: {changed} of {st.W * st.H} pixels change one entry short, 0 with depth + 1")
        assert changed >= st.W * st.H / 4 and short[3] == depth - 1
    sc = st.scene(flat, "C5")
    ref, _ = st.driver_rays(sc, rays["origins"], rays["dirs"], 64)
    exact, _ = st.driver_rays(sc, rays["origins"], rays["dirs"], depth + 1)
    short, _ = st.driver_rays(sc, rays["origins"], rays["dirs"], depth)
    changed = _differ(ref, short)
    print(f"mutants {kind}-{depth} rays: {changed} of {N_RAYS} records change one entry short, 0 with depth + 1")
    assert _differ(ref, exact) == 0 and changed >= N_RAYS / 4
    # the driver's records are the surface yardstick's (the oracle's own intersect_scene)
    rows = sf.oracle_hits(sc, rays["origins"], rays["dirs"])["rows"]
    assert (u32(rows.reshape(N_RAYS, 24)) == ref[:, 2:]).all()


@pytest.mark.parametrize("case", st.query_cases(), ids=lambda c: "-".join(str(x) for x in c))
def test_the_query_yardsticks_agree(oracle, native, case):
    """What test_gpu_stack.py compares the radiance, surface and shade queries
    with (stack_cases.query_case): on the spine rays the shade driver, given
    intersect_scene's own records, returns the trace's rgb bit for bit; most
    records are mesh hits and the radiance is not black."""
    q = st.query_case(*case)
    ok = q["kept"]
    assert ok.sum() >= 0.99 * len(ok)
    assert (u32(q["shaded"][ok][..., :3]) == u32(q["paths"][ok][..., :3])).all()
    assert not u32(q["shaded"][..., 3]).any()
    assert (q["records"][:, sf.KIND] == sf.MESH).sum() > len(ok) / 2
    assert np.any(q["paths"][ok][..., :3] != 0)


def test_the_oracle_itself_keeps_64_entries(oracle):
    """Built without the driver's macros the oracle has the reference's 64
    entries: a comb of depth 63 fills them, one of depth 64 is error -3."""
    assert st.oracle_render(st.scene(st.comb_tree(63)), 1, count=True)[3]["max_stack"] == 63
    with pytest.raises(RuntimeError, match="-3"):
        po.render(st.scene(st.comb_tree(64)), frames=1, times=[st.TIMES[0]], libm=po.LIBM_PORTABLE)


def test_the_depth_63_comb_is_a_valid_tree(native):
    """What initMesh refuses is a limit of the kernels' stacks, not of the tree format."""
    assert validate_flat(st.comb_tree(63)) == (63, 63)
    rays = st.spine_rays(st.comb_tree(63), 64)
    assert (flat_trace_rays(st.comb_tree(63), rays["origins"], rays["dirs"])["prim"] >= 0).sum() > 32


@pytest.mark.parametrize("where", st.TIES)
@pytest.mark.parametrize("depth", st.TIE_DEPTHS)
def test_ties(native, depth, where):
    """Coincident triangles whose root paths are `depth` levels each, or 1
    against `depth`: the host walk returns the one the reference's walk tests
    first, which an independent ordering (dfs_slots) names too."""
    flat = st.tie_comb(depth, where)
    assert validate_flat(flat)[0] == depth
    winner, loser = st.tie_slots(depth, where)
    assert (flat["verts"][winner:winner + 3] == flat["verts"][loser:loser + 3]).all()
    rays = st.spine_rays(flat, N_RAYS)
    o, d = rays["origins"], rays["dirs"]
    slots, V = flat_triangles(flat)
    acc, dist, _, _ = brute_force(V, o, d)
    hit, tmin = closest(acc, dist)
    got = flat_trace_rays(flat, o, d)
    col = {int(s): c for c, s in enumerate(slots)}
    tied = hit & acc[:, col[winner]] & (dist[:, col[winner]] == tmin)
    spine = tied & (rays["kind"] == "spine")
    assert spine.sum() >= N_RAYS / 4
    assert (got["prim"][spine] == winner).all()                     # down the axis child 0 is tested first
    for i in np.flatnonzero(tied):                                  # from the side either may be
        order = [s for s in dfs_slots(flat, o[i], d[i]) if acc[i, col[s]] and dist[i, col[s]] == tmin[i]]
        assert sorted(order) == sorted([winner, loser]) and got["prim"][i] == order[0], (i, order)
