"""Radiance from the caller's surface records (vrhip_shade_surface, vr_shade*.hip).

Two yardsticks.  The device's own: traceSurface followed by shadeSurface with
the same directions, seeds and samples is traceRadiance's rgb bit for bit, and
traceRadiance is pinned to the oracle in test_gpu_radiance.py.  And, for
records no ray produced (lightmap records, the mixed set M, alternating and
invalid records), tests/shade_driver.c, the oracle's trace restated with
bounce 0's hit given (tests/shade_cases.py; pinned to the oracle's trace in
test_shade_cpu.py): the results equal it bit for bit, compared as uint32, in
both traversal modes."""
import ctypes
import functools

import numpy as np
import pytest

import radiance_cases as rc
import shade_cases as sc
import surface_cases as sf
from device_mesh_cases import fresh
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, scenes

pytestmark = pytest.mark.gpu

_live = {}


def dev(a, dtype=np.float32):
    import torch
    a = np.array(a, dtype=dtype, order="C")              # a copy: the shared sets are read-only
    if dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda(0)


def dev_records(rec):
    import torch
    return torch.from_numpy(np.array(rec, dtype=np.uint32, order="C").view(np.float32)).cuda(0)


def renderer(name, mesh="shallow"):
    """One renderer per scene for the whole module; the tests leave its scene
    flags as they found them."""
    key = (name, mesh)
    if key not in _live:
        r = VRendererHIP(0)
        scenes.load_into(r, sf.scene_named(name, mesh))
        _live[key] = r
    return _live[key]


@pytest.fixture(scope="module", autouse=True)
def _renderers(native):
    yield
    for r in _live.values():
        r.cleanUp()
    _live.clear()


def shade(r, rec, d, s, samples=2):
    out = r.shadeSurface(dev_records(rec), dev(d), dev(s, np.uint32), samples=samples)
    assert out.is_cuda and tuple(out.shape) == (len(rec), 4) and str(out.dtype) == "torch.float32"
    return out.cpu().numpy()


def same(got, want, what):
    bad = np.flatnonzero((rc.u32(got) != rc.u32(want)).any(-1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} results differ (first {bad[:5].tolist()}: " \
                          f"{got[bad[:2]].tolist()} against {want[bad[:2]].tolist()})"


def same_or_nan(got, want, what):
    bad = np.flatnonzero(~sc.same_or_nan_in_both(got, want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} results differ (first {bad[:5].tolist()}: " \
                          f"{got[bad[:2]].tolist()} against {want[bad[:2]].tolist()})"


# ---- 1. the round trip ------------------------------------------------------------------------------
def check_round_trip(r, name, mesh, samples, what):
    scene = sf.scene_named(name, mesh)
    lit = False
    for which in sf.sets_of(scene):
        o, d, s = sc.ray_set(which, scene)
        do, dd, ds = dev(o), dev(d), dev(s, np.uint32)
        hits = r.traceSurface(do, dd)
        for k in samples:
            want = r.traceRadiance(do, dd, ds, samples=k).cpu().numpy()
            got = r.shadeSurface(hits if k != 2 else hits["record"], dd, ds, samples=k).cpu().numpy()
            assert tuple(got.shape) == (len(o), 4) and not rc.u32(got[:, 3]).any(), f"{what} set {which}: w is not +0"
            if sc.nan_case(name):
                same_or_nan(got[:, :3], want[:, :3], f"{what} set {which} samples {k}")
            else:
                same(got[:, :3], want[:, :3], f"{what} set {which} samples {k}")
            lit |= bool(np.any(np.nan_to_num(got[:, :3]) != 0))
    assert lit


@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("name", rc.COMBO_NAMES)
def test_round_trip(name, strict):
    r = renderer(name)
    r.set_strict_traversal(strict)
    try:
        check_round_trip(r, name, "shallow", sc.SAMPLES, f"{name} strict={strict}")
    finally:
        r.set_strict_traversal(False)


@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
def test_round_trip_on_the_deep_mesh(strict):
    """24-entry stacks: the class kernel, and the generic one in strict mode."""
    name = "cornell+mesh"
    r = renderer(name, "deep")
    assert 15 < r.bvh_info()[0] <= 23
    r.set_strict_traversal(strict)
    try:
        check_round_trip(r, name, "deep", sc.SAMPLES, f"deep {name} strict={strict}")
    finally:
        r.set_strict_traversal(False)


@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("name", rc.SHADING_NAMES)
def test_round_trip_on_shading_scenes(name, strict):
    """Maps of odd shapes, zero tangents, the example sphere with maps, and a
    scene with NaN normals (tests/shading_cases.py), the NaN case equal or NaN in both."""
    r = renderer(name)
    r.set_strict_traversal(strict)
    try:
        check_round_trip(r, name, "shallow", sc.SAMPLES, f"{name} strict={strict}")
    finally:
        r.set_strict_traversal(False)


# ---- 2. records no ray produced, against the driver --------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("what", ["lightmap", "mixed"])
@pytest.mark.parametrize("name", rc.COMBO_NAMES)
def test_edited_records_against_the_driver(oracle, name, what, strict):
    r = renderer(name)
    scene = sf.scene_named(name)
    r.set_strict_traversal(strict)
    try:
        for which in sf.sets_of(scene):
            rec, d, s, paths, ok = sc.reference(name, which, what)
            for k in sc.SAMPLES:
                got = shade(r, rec, d, s, k)
                same(got[ok], sc.result_of(paths, k)[ok], f"{name} {what} strict={strict} set {which} samples {k}")
            if what == "lightmap":                       # the direction plays no part in a hit record
                hit = rec[:, sf.KIND] != sf.NONE
                same(shade(r, rec, d[::-1], s, 2)[hit & ok], got_2(paths)[hit & ok], f"{name} set {which} reversed directions")
        # a miss made a hit: a zero normal, NaN by the reference's arithmetic
        rec, d, s, _, _ = sc.reference(name, "D")
        one, i = sc.miss_made_a_hit(rec)
        want = sc.result_of(sc.driver_paths(scene, one, d[i:i + 1], s[i:i + 1], 2), 2)
        same_or_nan(shade(r, one, d[i:i + 1], s[i:i + 1], 2), want, f"{name} strict={strict} a miss made a hit")
    finally:
        r.set_strict_traversal(False)


def got_2(paths):
    return sc.result_of(paths, 2)


# ---- 3. diffuseRecords ---------------------------------------------------------------------------------
def test_diffuse_records(oracle):
    import torch
    name = "cornell+mesh"
    r = renderer(name)
    scene = sf.scene_named(name)
    rec, d, s, paths, ok = sc.reference(name, "C", "lightmap")
    hit = rec[:, sf.KIND] != sf.NONE
    rec, d, s, paths, ok = rec[hit], d[hit], s[hit], paths[hit], ok[hit]
    f = sf.floats(rec)
    pts, nrm = dev(f[:, sf.POSITION]), dev(f[:, sf.NORMAL])
    made = r.diffuseRecords(pts, nrm * 3.0)              # normalised there
    assert made.is_cuda and tuple(made.shape) == (len(rec), 28) and made.dtype == torch.float32
    m = np.ascontiguousarray(made.cpu().numpy()).view(np.uint32)
    unit = (nrm * 3.0) / (nrm * 3.0).norm(dim=1, keepdim=True)
    want = rec.copy()
    want[:, sf.T] = 0
    want[:, sf.KIND], want[:, sf.PRIM] = sf.MESH, sf.MISS                  # prim -1
    want[:, [sf.BARY_U, sf.BARY_V, sf.TEX_U, sf.TEX_V]] = 0
    want[:, sf.TANGENT] = 0
    want[:, sf.NORMAL] = rc.u32(unit.cpu().numpy())
    assert (m == want).all()
    # a unit normal stays one: under ten roundings (the scaling, the norm's products, sums and root, the division),
    # each at most 2^-24 of a component that is at most 1
    assert np.abs(sf.floats(m)[:, sf.NORMAL] - f[:, sf.NORMAL]).max() <= 10 * 2.0 ** -24
    # what the library makes of them is what the yardstick makes of them
    got = r.shadeSurface(made, -nrm, dev(s, np.uint32), samples=5).cpu().numpy()
    mine = sc.driver_paths(scene, m, -f[:, sf.NORMAL], s, 5)
    fin = sc.kept(mine)
    same(got[fin], sc.result_of(mine, 5)[fin], "diffuseRecords against the driver")
    # and, where torch's normalisation hands the oracle's own unit normal back, the edited records' result
    plain = r.diffuseRecords(pts, nrm)
    eq = (np.ascontiguousarray(plain.cpu().numpy()).view(np.uint32)[:, sf.NORMAL] == rec[:, sf.NORMAL]).all(-1)
    print(f"{int(eq.sum())} of {len(eq)} normals come back bit for bit")
    assert eq.any()
    got = r.shadeSurface(plain, -nrm, dev(s, np.uint32), samples=5).cpu().numpy()
    same(got[eq & ok], sc.result_of(paths, 5)[eq & ok], "diffuseRecords against the edited records")
    col = r.diffuseRecords(pts, nrm, color=(0.25, 0.5, 1.0)).cpu().numpy()
    assert (col[:, sf.COLOR] == np.array([0.25, 0.5, 1.0], np.float32)).all()
    per = r.diffuseRecords(pts, nrm, color=pts.abs()).cpu().numpy()
    assert (per[:, sf.COLOR] == np.abs(f[:, sf.POSITION])).all()
    for bad in (dict(color=torch.ones(3)), dict(color=torch.ones((2, 3), device="cuda:0"))):
        with pytest.raises(ValueError):
            r.diffuseRecords(pts, nrm, **bad)


# ---- 4. refill and tails -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def alternating(name, n, k_max, seed=20241022):
    """n records alternating miss and hit, so that neighbouring lanes retire
    out of step: the misses and the hits of the scene's sets A and D, cycled;
    their directions; seeds from a fixed generator; the driver's paths."""
    scene = sf.scene_named(name)
    recs, dirs = [], []
    for which in ("A", "D"):
        rec, d, _, _, _ = sc.reference(name, which)
        recs.append(rec)
        dirs.append(d)
    rec, d = np.concatenate(recs), np.concatenate(dirs)
    miss, hit = np.flatnonzero(rec[:, sf.KIND] == sf.NONE), np.flatnonzero(rec[:, sf.KIND] != sf.NONE)
    assert len(miss) >= 16 and len(hit) >= 512
    i = np.arange(n)
    idx = np.where(i % 2 == 0, miss[(i // 2) % len(miss)], hit[(i // 2) % len(hit)])
    s = np.random.default_rng(seed).integers(0, 2**32, (n, 2), dtype=np.uint64).astype(np.uint32)
    rec, d = np.ascontiguousarray(rec[idx]), np.ascontiguousarray(d[idx])
    paths = sc.driver_paths(scene, rec, d, s, k_max)
    return rec, d, s, paths, sc.finite(paths)


def shade_with_canary(r, rec, d, s, samples, extra=4):
    """Through the C ABI into a buffer of n + extra rows; the rows after n must keep their canary."""
    import torch
    n = len(rec)
    out = torch.full((n + extra, 4), -7.5, dtype=torch.float32, device="cuda:0")
    h, dd, ss = dev_records(rec), dev(d), dev(s, np.uint32)
    torch.cuda.synchronize()
    p = lambda x: ctypes.c_void_p(x.data_ptr())                            # noqa: E731
    assert r._lib.vrhip_shade_surface(r._ctx, p(h), p(dd), p(ss), n, samples, p(out)) == 0
    out = out.cpu().numpy()
    assert (out[n:] == -7.5).all(), "rows after the last record were written"
    return out[:n]


@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 193, 1000])
def test_record_counts_and_lanes_out_of_step(oracle, n, strict):
    name = "cornell+mesh"
    r = renderer(name)
    rec, d, s, paths, ok = alternating(name, 1000, 8)
    assert ok.sum() >= (1.0 - sc.MAX_DROPPED) * len(ok)
    rec, d, s, paths, ok = rec[:n], d[:n], s[:n], paths[:n], ok[:n]
    r.set_strict_traversal(strict)
    try:
        for k in (1, 3, 8):
            got = shade_with_canary(r, rec, d, s, k)
            same(got[ok], sc.result_of(paths, k)[ok], f"{n} records, samples {k}")
            assert not rc.u32(got[:, 3]).any()
    finally:
        r.set_strict_traversal(False)


def test_order_and_repeats(oracle):
    """A permutation of the records gives the permuted result, and two calls
    are equal: a result does not depend on the lane or wave that took it."""
    name = "cornell+mesh"
    r = renderer(name)
    rec, d, s, paths, ok = alternating(name, 1000, 8)
    a = shade(r, rec, d, s, 3)
    same(shade(r, rec, d, s, 3), a, "two calls")
    perm = np.random.default_rng(5).permutation(len(rec))
    same_or_nan(shade(r, rec[perm], d[perm], s[perm], 3), a[perm], "a permutation")
    same(a[ok], sc.result_of(paths, 3)[ok], "the yardstick")


def test_around_the_slice_length(oracle):
    name = "cornell+mesh"
    r = renderer(name)
    L = sc.slice_length()
    rec, d, s, paths, ok = alternating(name, 2 * L + 1, 2, seed=3)
    for n in (L - 1, L, L + 1, 2 * L + 1):
        got = shade_with_canary(r, rec[:n], d[:n], s[:n], 2)
        same(got[ok[:n]], sc.result_of(paths, 2)[:n][ok[:n]], f"{n} records, slices of {L}")


def test_more_records_than_a_resident_set(oracle):
    import torch
    name = "cornell+example"
    r = renderer(name)
    # the launcher's resident set: VR_SPHERE_MIN_WAVES (6) blocks of four waves on each CU, a slice per wave
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (6 * cus + 3) * 4 * sc.slice_length() + 77
    rec, d, s, paths, ok = sc.reference(name, "A")
    base = len(rec)
    idx = torch.arange(n, device="cuda:0") % base
    got = r.shadeSurface(dev_records(rec)[idx].contiguous(), dev(d)[idx].contiguous(), dev(s, np.uint32)[idx].contiguous(),
                         samples=1)
    assert bool((got.view(torch.int32) == got.view(torch.int32)[idx]).all()), "record i against record i mod 1024"
    same(got[:base].cpu().numpy()[ok], sc.result_of(paths, 1)[ok], "the first 1,024 records")


def test_the_most_samples(oracle):
    """8 records at 4,096 paths each: a lane's sum over its record's whole seed stream."""
    name = "cornell+mesh"
    r = renderer(name)
    rec, d, s, _, _ = alternating(name, 1000, 1)
    rec, d, s = rec[100:108], d[100:108], s[100:108]
    paths = sc.driver_paths(sf.scene_named(name), rec, d, s, 4096)
    assert sc.finite(paths).all()
    same(shade(r, rec, d, s, 4096), sc.result_of(paths, 4096), "8 records, 4096 samples")


# ---- 5. invalid records -----------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
def test_invalid_records_in_a_batch(oracle, strict):
    name = "cornell+mesh"
    r = renderer(name)
    rec, d, s, paths, ok = (np.array(a[:200]) for a in sc.reference(name, "C", "mixed"))
    hit = np.flatnonzero(rec[:, sf.KIND] != sf.NONE)
    r.set_strict_traversal(strict)
    try:
        clean = shade(r, rec, d, s, 2)
        rows = []
        for j in range(8):                               # in rotation, so that invalid and valid lanes mix in both waves
            b = hit[5 * j: 5 * j + 5] if j < 4 else hit[-5 * (j - 3): len(hit) - 5 * (j - 4)]
            d[b[0], 1] = np.nan
            d[b[1], 2] = -np.inf
            d[b[2]] = 0.0
            rec[b[3], sf.KIND] = 5
            rec[b[4], sf.TYPE] = 3
            rows += b.tolist()
        d[hit[40]] = (3e19, -3e19, 3e19)                 # finite, the squared length overflows
        rows.append(int(hit[40]))
        got = shade(r, rec, d, s, 2)
    finally:
        r.set_strict_traversal(False)
    assert len(set(rows)) == 41 and not rc.u32(got[rows]).any()             # exactly {0, 0, 0, 0}
    rest = np.setdiff1d(np.arange(len(rec)), rows)
    same_or_nan(got[rest], clean[rest], "the valid records of the batch")
    same(clean[ok], sc.result_of(paths, 2)[ok], "the batch before it was spoilt")
    assert np.any(clean[rows] != 0)
    # a miss needs no type, and the words the call does not read may hold anything
    one, dd, ss, _, _ = (np.array(a) for a in sc.reference(name, "D"))
    base = shade(r, one, dd, ss, 2)
    miss = one[:, sf.KIND] == sf.NONE
    assert 16 <= miss.sum() <= len(one) - 16
    one[miss, sf.TYPE] = 77
    one[~miss, sf.KIND] = 1 + np.arange((~miss).sum()) % 4
    one[:, [sf.T, sf.PRIM, sf.BARY_U, sf.BARY_V, sf.PAD0, sf.TEX_U, sf.TEX_V, sf.PAD1]] = 0x7FC00000
    same(shade(r, one, dd, ss, 2), base, "another kind of hit, misses with a type, NaNs in the unread words")


# ---- 6. nothing else moves -----------------------------------------------------------------------------------
def test_a_call_leaves_everything_else_alone(oracle):
    name = "cornell+mesh"
    scene = sf.scene_named(name)
    rec, d, s, _, _ = sc.reference(name, "B", "mixed")
    state = {}
    for query in (False, True):
        q = VRendererHIP(0)
        scenes.load_into(q, scene)
        q.render(frames=2, times=[11, 12])
        before = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount(), q.export_mesh_flat())
        if query:
            a, b = shade(q, rec, d, s, 2), shade(q, rec, d, s, 2)
            same_or_nan(a, b, "two calls")
            after = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount(), q.export_mesh_flat())
            for x, y in zip(before[:3], after[:3]):
                assert x.tobytes() == y.tobytes()
            assert before[3] == after[3] == 2
            assert all(before[4][k].tobytes() == after[4][k].tobytes() for k in before[4])
        q.render(frames=1, times=[13])
        state[query] = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount())
        q.cleanUp()
    for x, y in zip(state[False][:3], state[True][:3]):
        assert x.tobytes() == y.tobytes()
    assert state[False][3] == state[True][3] == 3


def test_between_unsynchronised_renders_of_a_session(oracle):
    name = "cornell+mesh"
    scene = sf.scene_named(name)
    rec, d, s, paths, ok = sc.reference(name, "B", "mixed")
    images = {}
    for query in (False, True):
        q = VRendererHIP(0)
        scenes.load_into(q, scene)
        q.set_service(1)
        q.render(frames=2, times=[11, 12], sync=False)
        if query:
            s0 = q.service_info()["sessions"]
            same(shade(q, rec, d, s, 2)[ok], sc.result_of(paths, 2)[ok], "inside a session")
        q.render(frames=2, times=[13, 14], sync=False)
        q.sync()
        if query:
            assert q.service_info()["sessions"] > s0 >= 1        # the call closed the first session
        assert q.getFrameCount() == 4
        images[query] = (q.read_accum(), q.read_rgba8(), q.read_depth8())
        q.cleanUp()
    for a, b in zip(images[False], images[True]):
        assert a.tobytes() == b.tobytes()
    assert np.any(images[True][0][..., :3] != 0)


def test_scene_toggles(oracle):
    """useCornellBox / useExampleSphere on one renderer: the records are traced
    through the scene as it is now, the mesh ignored while the example sphere is on."""
    name = "cornell+mesh"
    base = sf.scene_named(name)
    rec, d, s, _, _ = sc.reference(name, "B", "mixed")
    q = VRendererHIP(0)
    scenes.load_into(q, base)
    seen = set()
    try:
        for cornell, example in ((True, True), (False, True), (False, False), (True, False)):
            q.useCornellBox(cornell)
            q.useExampleSphere(example)
            scene = dict(base, cornell=cornell, example_sphere=example)
            paths = sc.driver_paths(scene, rec, d, s, 2)
            ok = sc.kept(paths)
            got = shade(q, rec, d, s, 2)
            same(got[ok], sc.result_of(paths, 2)[ok], f"cornell={cornell} example={example}")
            seen.add(got[ok].tobytes())
    finally:
        q.cleanUp()
    assert len(seen) == 4


# ---- 7. refusals ------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    import torch
    rec, d, s, _, _ = sc.reference("cornell+example", "B")
    h, d, s = dev_records(rec[:64]), dev(d[:64]), dev(s[:64], np.uint32)
    q = VRendererHIP([0])                                # a multi-device context of one device
    q.init(64, 48)
    with pytest.raises(VRHIPError) as e:
        q.shadeSurface(h, d, s)
    assert e.value.code == -1 and "multi-device" in str(e.value)
    q.cleanUp()
    q = fresh()                                          # HDRI mode, no environment
    with pytest.raises(VRHIPError) as e:
        q.shadeSurface(h, d, s)
    assert e.value.code == -3
    assert tuple(q.shadeSurface(h[:0], d[:0], s[:0]).shape) == (0, 4)       # nothing to do comes first, as in vrhip_render
    q.useCornellBox(True)                                # a scene without a mesh
    want = q.shadeSurface(h, d, s).cpu().numpy()
    assert np.isfinite(want).all() and np.any(want[:, :3] != 0)
    for samples in (0, 4097):
        with pytest.raises(VRHIPError) as e:
            q.shadeSurface(h, d, s, samples=samples)
        assert e.value.code == -1
    p = lambda x: ctypes.c_void_p(x.data_ptr())                            # noqa: E731
    out = torch.zeros((65, 4), dtype=torch.float32, device="cuda:0")
    h65 = torch.zeros((65, 28), dtype=torch.float32, device="cuda:0")
    h65[:64] = h
    torch.cuda.synchronize()
    f = q._lib.vrhip_shade_surface
    assert f(q._ctx, p(h), p(d), p(s), 64, 2, ctypes.c_void_p(out.data_ptr() + 4)) == -1      # misaligned result
    assert f(q._ctx, ctypes.c_void_p(h65.data_ptr() + 8), p(d), p(s), 64, 2, p(out)) == -1    # misaligned records
    assert f(q._ctx, None, p(d), p(s), 64, 2, p(out)) == -1
    assert f(q._ctx, p(h), None, p(s), 64, 2, p(out)) == -1
    assert f(q._ctx, p(h), p(d), None, 64, 2, p(out)) == -1
    assert f(q._ctx, p(h), p(d), p(s), 64, 2, None) == -1
    assert f(q._ctx, p(h), p(d), p(s), 64, 0, p(out)) == -1
    assert f(q._ctx, p(h), p(d), p(s), 64, 4097, p(out)) == -1
    assert f(None, p(h), p(d), p(s), 64, 2, p(out)) == -1
    assert not out.cpu().numpy().any()                   # nothing written by a refused call
    assert f(q._ctx, None, None, None, 0, 2, None) == 0
    wrong = [dict(hits=h.cpu(), dirs=d), dict(hits=h, dirs=d.double()), dict(hits=h, dirs=d[:-1]),
             dict(hits=h[:, :27].contiguous(), dirs=d), dict(hits=h.double(), dirs=d), dict(hits=h, dirs=d, seeds=s[:-1]),
             dict(hits=h, dirs=d, seeds=s.float()), dict(hits=h, dirs=d, seeds=s[:, :1].contiguous()),
             dict(hits=h, dirs=d, seeds=s.cpu()), dict(hits=None, dirs=d), dict(hits=h, dirs=None), dict(hits={}, dirs=d)]
    for kw in wrong:                                     # device, dtype, shape, missing
        with pytest.raises(ValueError):
            q.shadeSurface(**kw)
    drawn = q.shadeSurface(h, d, samples=4)              # seeds drawn on the device
    assert tuple(drawn.shape) == (64, 4) and np.isfinite(drawn.cpu().numpy()).all()
    again = q.shadeSurface(h, d, s).cpu().numpy()
    assert (rc.u32(again) == rc.u32(want)).all()
    assert q.shadeSurface(h, d, s, samples=4096).shape[0] == 64            # the upper bound itself
    q.cleanUp()
