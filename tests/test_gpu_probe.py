"""Probe radiance on spherical harmonics (vrhip_probe_sh, vr_probe*.hip) and
the irradiance at a normal (vrhip_sh_irradiance).

Every comparison is made as uint32 over all 28 words of a record (a
coefficient may instead be NaN in both).  Two yardsticks feed
tests/probe_driver.c, the definition restated in C: the oracle's own trace of
the expanded rays (tests/probe_cases.py), and the library's traceRadiance on
the expanded rays, which is itself pinned to the oracle
(test_gpu_radiance.py)."""
import ctypes
import math

import numpy as np
import pytest

import flag_lattice as fl
import probe_cases as pc
import radiance_cases as rc
import stack_cases as st
import surface_cases as sf
from device_mesh_cases import fresh
from vrenderer_pathtracer_amd import VRendererHIP, VRHIPError, scenes

pytestmark = pytest.mark.gpu

WALKS = [False, True]
_live = {}


def dev(a, dtype=np.float32):
    import torch
    a = np.array(a, dtype=dtype, order="C")              # a copy: the shared sets are read-only
    if dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda(0)


def renderer(name, mesh="shallow"):
    """One renderer per scene for the whole module; the tests leave its scene
    flags as they found them."""
    key = (name, mesh)
    if key not in _live:
        r = VRendererHIP(0)
        scenes.load_into(r, fl.scene_of(rc.combo_of(name), mesh))
        _live[key] = r
    return _live[key]


@pytest.fixture(scope="module", autouse=True)
def _renderers(native):
    yield
    for r in _live.values():
        r.cleanUp()
    _live.clear()


def probe(r, pts, d, w, ps, ds, samples=2):
    out = r.probeSH(dev(pts), dev(d), None if w is None else dev(w), dev(ps, np.uint32), dev(ds, np.uint32), samples=samples)
    assert out.is_cuda and tuple(out.shape) == (len(pts), 28) and str(out.dtype) == "torch.float32"
    return out.cpu().numpy().view(np.uint32)


def by_trace_radiance(r, pts, d, w, ps, ds, samples=2):
    """The records by the composition the call replaces: traceRadiance on the
    expanded rays, then the driver."""
    o, dd, s = pc.expand(pts, d, ps, ds)
    rec = r.traceRadiance(dev(o), dev(dd), dev(s, np.uint32), samples=samples).cpu().numpy()
    return pc.project(rec.reshape(len(pts), len(d), 4), d, w, pc.valid_rays(pts, d))


def same(got, want, what):
    bad = np.flatnonzero(~pc.same_words(got, want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ (first {bad[:5].tolist()}: " \
                          f"{got[bad[:1]].tolist()} against {want[bad[:1]].tolist()})"


def strictly(r, strict, fn):
    r.set_strict_traversal(strict)
    try:
        return fn()
    finally:
        r.set_strict_traversal(False)


# ---- 1. against the oracle and the driver ----------------------------------------------------
@pytest.mark.parametrize("strict", WALKS, ids=["culled", "strict"])
@pytest.mark.parametrize("name", rc.COMBO_NAMES)
def test_against_the_oracle(oracle, name, strict):
    r = renderer(name)
    pts, d, _, ps, ds = pc.probe_set()

    def run():
        for n in pc.N_DIRS:
            for k in rc.SAMPLES:
                want = pc.oracle_records(name, n, k)
                ok = pc.finite_probes(want)
                got = probe(r, pts, d[:n], pc.weights_for(n), ps, ds[:n], k)
                same(got[ok], want[ok], f"{name} strict={strict} n_dirs {n} samples {k}")
                same(got[~ok], want[~ok], f"{name} strict={strict} n_dirs {n} samples {k}, non-finite probes")
                assert (got[:, 27] == n).all()
        assert np.any(want[:, :27] != 0)
    strictly(r, strict, run)


# ---- 2. against traceRadiance on the expanded rays ----------------------------------------------
def big_set():
    rng = np.random.default_rng(77)
    pts = rc.ray_set("B")[0][:300]
    d, w = scenes.probe_directions(257)
    d = (d.astype(np.float64) * rng.uniform(0.5, 2.0, (257, 1))).astype(np.float32)
    ps = rng.integers(0, 2**32, (300, 2), dtype=np.uint64).astype(np.uint32)
    ds = rng.integers(0, 2**32, (257, 2), dtype=np.uint64).astype(np.uint32)
    return np.array(pts), d, w, ps, ds


@pytest.mark.parametrize("strict", WALKS, ids=["culled", "strict"])
def test_against_trace_radiance(strict):
    r = renderer("cornell+mesh")
    pts, d, w, ps, ds = big_set()

    def run():
        none = probe(r, pts, d, None, ps, ds)
        same(none, by_trace_radiance(r, pts, d, None, ps, ds), "no weights")
        assert (none == probe(r, pts, d, w, ps, ds)).all(), "explicit weights equal to the default"
        assert np.isfinite(none.view(np.float32)[:, :27]).all() and np.any(none[:, :27] != 0)
        odd = w.copy()
        odd[3], odd[64], odd[200:231], odd[256] = np.nan, np.inf, 0.0, 0.0
        got = probe(r, pts, d, odd, ps, ds)
        same(got, by_trace_radiance(r, pts, d, odd, ps, ds), "a NaN weight, an inf weight and weights of 0")
        assert np.isnan(got.view(np.float32)[:, :27]).all() and (got[:, 27] == 257).all()
        odd[3] = odd[64] = 0.25
        got = probe(r, pts, d, odd, ps, ds)
        same(got, by_trace_radiance(r, pts, d, odd, ps, ds), "weights of 0")
        assert np.isfinite(got.view(np.float32)[:, :27]).all()
    strictly(r, strict, run)


# ---- 3. invalid rays ---------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", WALKS, ids=["culled", "strict"])
def test_invalid_rays(strict):
    r = renderer("cornell+mesh")
    pts, d, w, ps, ds = big_set()
    pts, d, w = pts[:130].copy(), d.copy(), w.copy()
    ps = ps[:130]
    pts[0, 1], pts[31, 0], pts[63, 2], pts[64] = np.nan, np.inf, -np.inf, np.nan      # wholly invalid probes
    d[64], d[95, 2], d[127] = 0.0, np.nan, (3e19, -3e19, 3e19)        # slots 0, 31 and 63 of block 1
    d[128:192] = np.where(np.arange(64)[:, None] % 3 == 0, 0.0, np.nan).astype(np.float32) * np.ones(3, np.float32)   # block 2, wholly
    w[95] = np.nan                                          # on an invalid direction: must not reach any sum
    valid = pc.valid_rays(pts, d)
    assert not valid[:, 128:192].any() and not valid[[0, 31, 63, 64]].any() and valid[1, :64].all()

    def run():
        got = probe(r, pts, d, w, ps, ds)
        same(got, by_trace_radiance(r, pts, d, w, ps, ds), "invalid points and directions")
        assert (got[:, 27] == valid.sum(-1)).all()
        assert not got[[0, 31, 63, 64]].any()               # count 0 and every coefficient +0
        assert (got[1, 27] == 257 - 3 - 64) and np.isfinite(got.view(np.float32)[1, :27]).all()
        # a call whose every block is invalid but the tail
        only_tail = probe(r, pts[:3], d[128:193], None, ps[:3], ds[128:193])
        same(only_tail, by_trace_radiance(r, pts[:3], d[128:193], None, ps[:3], ds[128:193]), "one valid lane in the tail")
        assert list(only_tail[:, 27]) == [0, 1, 1]
    strictly(r, strict, run)


# ---- 4. independence from decomposition -----------------------------------------------------------------
def test_independent_of_the_split_and_repeatable():
    r = renderer("mesh+tex_d+tex_n+tex_s")
    pts, d, w, ps, ds = big_set()
    whole = probe(r, pts, d, w, ps, ds, 3)
    assert (whole == probe(r, pts, d, w, ps, ds, 3)).all(), "two calls"
    h = len(pts) // 2
    halves = np.concatenate([probe(r, pts[:h], d, w, ps[:h], ds, 3), probe(r, pts[h:], d, w, ps[h:], ds, 3)])
    assert (whole == halves).all(), "[0, n) against [0, n/2) and [n/2, n)"
    one = np.concatenate([probe(r, pts[i:i + 1], d, w, ps[i:i + 1], ds, 3) for i in (0, 149, 299)])
    assert (whole[[0, 149, 299]] == one).all(), "a probe on its own"
    assert np.any(whole[:, :27] != 0)


def test_more_items_than_a_resident_set():
    """The grid-stride loop: more (probe, block) items than one resident set of waves."""
    import torch
    r = renderer("cornell+example")
    pts, d, w, ps, ds = big_set()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 6 * cus * 4 + 77                                     # VR_SPHERE_MIN_WAVES (6) blocks of 4 waves on each CU, and some
    idx = np.arange(n) % 50
    got = probe(r, pts[idx], d[:65], None, ps[idx], ds[:65])
    assert (got == got[idx]).all(), "record i against record i mod 50"
    same(got[:50], by_trace_radiance(r, pts[:50], d[:65], None, ps[:50], ds[:65]), "the first 50 records")


# ---- 5. a full traversal stack -----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C2", "C3"])
@pytest.mark.parametrize("depth", [15, 23, 30, 62])
def test_full_traversal_stack(oracle, depth, cfg):
    """The probes sit on the disc the spine rays start from and a block of
    directions looks down the spine: every lane's walk fills the stack of the
    kernel built for this depth to its last entry, in both walks."""
    flat = st.tree("comb", depth)
    rays = st.rays_of("comb", depth, 256)
    spine = np.flatnonzero(rays["kind"] == "spine")
    pts = np.array(rays["origins"][spine[:6]])
    d = np.array(rays["dirs"][spine[:70]])                    # a full block and a tail of six
    rng = np.random.default_rng(depth)
    ps = rng.integers(0, 2**32, (len(pts), 2), dtype=np.uint64).astype(np.uint32)
    ds = rng.integers(0, 2**32, (len(d), 2), dtype=np.uint64).astype(np.uint32)
    o, dd, s = pc.expand(pts, d, ps, ds)
    top = [st.high_water(flat, o[i], sf.normalised(dd[i:i + 1])[0]) for i in range(0, len(o), 7)]
    assert max(top) == depth and np.mean(np.array(top) == depth) > 0.5
    sc = st.scene(flat, cfg)
    rec = rc.oracle_radiance(sc, o, dd, s, 2).reshape(len(pts), len(d), 4)
    want = pc.project(rec, d, None, pc.valid_rays(pts, d))
    assert np.isfinite(want.view(np.float32)[:, :27]).all() and np.any(want[:, :27] != 0)
    r = VRendererHIP(0)
    try:
        scenes.load_into(r, sc)
        assert r.bvh_info()[0] == depth
        for strict in WALKS:
            got = strictly(r, strict, lambda: probe(r, pts, d, None, ps, ds))
            same(got, want, f"comb {depth} {cfg} strict={strict}")
    finally:
        r.cleanUp()


# ---- 6. shIrradiance ------------------------------------------------------------------------------------------
def test_sh_irradiance():
    import torch
    r = renderer("cornell+mesh")
    rng = np.random.default_rng(9)
    m, n = 37, 300
    sh = rng.normal(0.0, 2.0, (m, 28)).astype(np.float32)
    sh[5, 4], sh[6, 9] = np.nan, np.inf
    nrm = rng.normal(0.0, 1.0, (n, 3)).astype(np.float32)    # used as given: not unit
    nrm[7], nrm[8, 1], nrm[9] = 0.0, np.nan, (1e30, -1e30, 1e30)
    idx = rng.integers(0, m, n).astype(np.uint32)
    idx[[0, 100, 299]] = [m, 0xFFFFFFFF, m + 1]               # out of range
    got = r.shIrradiance(dev(sh), dev(nrm), dev(idx, np.uint32))
    assert got.is_cuda and tuple(got.shape) == (n, 4) and str(got.dtype) == "torch.float32"
    got = got.cpu().numpy()
    want = pc.irradiance(sh, nrm, idx)
    ok = (pc.u32(got) == pc.u32(want)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), np.flatnonzero(~ok.all(-1))[:5]
    assert not pc.u32(got[[0, 100, 299]]).any() and not pc.u32(got[:, 3]).any()
    assert np.isfinite(got[10:100]).any() and np.isnan(got).any()
    # without an index: record q at normal q
    got = r.shIrradiance(dev(sh), dev(nrm[:m])).cpu().numpy()
    want = pc.irradiance(sh, nrm[:m])
    assert ((pc.u32(got) == pc.u32(want)) | (np.isnan(got) & np.isnan(want))).all()
    # m = 1
    got = r.shIrradiance(dev(sh[:1]), dev(nrm), dev(np.zeros(n, np.uint32), np.uint32)).cpu().numpy()
    want = pc.irradiance(sh[:1], nrm, np.zeros(n, np.uint32))
    assert ((pc.u32(got) == pc.u32(want)) | (np.isnan(got) & np.isnan(want))).all()
    got = r.shIrradiance(dev(sh[:1]), dev(nrm[:1])).cpu().numpy()
    assert (pc.u32(got) == pc.u32(pc.irradiance(sh[:1], nrm[:1]))).all()
    assert tuple(r.shIrradiance(dev(sh), dev(nrm[:0]), dev(idx[:0], np.uint32)).shape) == (0, 4)
    for kw in (dict(sh=dev(sh), normals=dev(nrm)), dict(sh=dev(sh[:, :27]), normals=dev(nrm[:m])),
               dict(sh=dev(sh), normals=dev(nrm), index=dev(idx[:-1], np.uint32)),
               dict(sh=dev(sh).cpu(), normals=dev(nrm[:m])), dict(sh=dev(sh), normals=dev(nrm[:m]).double()),
               dict(sh=None, normals=dev(nrm)), dict(sh=dev(sh), normals=dev(nrm), index=dev(idx).float())):
        with pytest.raises(ValueError):
            r.shIrradiance(**kw)
    p = lambda x: ctypes.c_void_p(x.data_ptr())             # noqa: E731
    s_, n_, out = dev(sh), dev(nrm), torch.zeros((n + 1, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    lib = r._lib
    assert lib.vrhip_sh_irradiance(r._ctx, p(s_), m, None, p(n_), n, p(out)) == -1                   # no index, n != m
    assert lib.vrhip_sh_irradiance(r._ctx, None, m, None, p(n_), m, p(out)) == -1
    assert lib.vrhip_sh_irradiance(r._ctx, p(s_), m, None, None, m, p(out)) == -1
    assert lib.vrhip_sh_irradiance(r._ctx, p(s_), m, None, p(n_), m, None) == -1
    assert lib.vrhip_sh_irradiance(r._ctx, p(s_), m, None, p(n_), m, ctypes.c_void_p(out.data_ptr() + 4)) == -1
    assert lib.vrhip_sh_irradiance(r._ctx, None, 0, None, None, 0, None) == 0
    assert not out.cpu().numpy().any()


# ---- 7. the round trip ---------------------------------------------------------------------------------------
def test_round_trip_under_a_constant_environment():
    """A constant HDRI and no mesh: every ray that misses the scene's two small
    spheres returns the same radiance L, and shIrradiance(probeSH(...)) is the
    driver's value bit for bit and pi L within the CPU test's bound."""
    k = 256
    d, w = scenes.probe_directions(k)
    u = pc.unit64(d)
    # a probe of ray set B from which every direction passes both small spheres (radius 3.5) by 1 at least
    centres = np.array([[15.0, 0.0, 15.0], [25.0, 0.0, 15.0]])
    pts = []
    for c in np.array(rc.ray_set("B")[0], np.float64):
        oc = centres - c
        along = oc @ u.T
        gap = np.sqrt(np.maximum(0.0, (oc * oc).sum(-1)[:, None] - along * along))
        if ((along < 0) | (gap > 4.5)).all():
            pts.append(c)
        if len(pts) == 3:
            break
    pts = np.array(pts, np.float32)
    assert len(pts) == 3
    rng = np.random.default_rng(4)
    ps = rng.integers(0, 2**32, (3, 2), dtype=np.uint64).astype(np.uint32)
    ds = rng.integers(0, 2**32, (k, 2), dtype=np.uint64).astype(np.uint32)
    r = fresh()
    try:
        env = np.zeros((8, 16, 4), np.float32)
        env[...] = (0.75, 1.5, 0.03125, 1.0)
        r.loadHDR(env)
        o, dd, s = pc.expand(pts, d, ps, ds)
        rec = r.traceRadiance(dev(o), dev(dd), dev(s, np.uint32), samples=2).cpu().numpy()
        L = rec[0, :3].copy()
        assert (pc.u32(rec[:, :3]) == pc.u32(L)).all() and (L > 0).all(), "every ray escapes to the same radiance"
        sh = r.probeSH(dev(pts), dev(d), None, dev(ps, np.uint32), dev(ds, np.uint32))
        want = pc.project(rec.reshape(3, k, 4), d, None, pc.valid_rays(pts, d))
        same(sh.cpu().numpy().view(np.uint32), want, "probeSH")
        nrm = pc.unit64(rng.normal(size=(3, 3))).astype(np.float32)
        E = r.shIrradiance(sh, dev(nrm)).cpu().numpy()
        assert (pc.u32(E) == pc.u32(pc.irradiance(want, nrm))).all()
    finally:
        r.cleanUp()
    exact, abs_sum = pc.project64(rec.reshape(3, k, 4), d, None)
    ideal = np.zeros((9, 3))
    ideal[0] = 2.0 * math.sqrt(math.pi) * L.astype(np.float64)
    for i in range(3):
        tol = pc.bound_of(abs_sum[i], k) + np.abs(exact[i] - ideal)
        got = want[i].view(np.float32)[:27].reshape(9, 3).astype(np.float64)
        assert (np.abs(got - ideal) <= tol).all()
        etol = pc.irradiance_bound(nrm[i:i + 1], got, tol, L)
        assert (np.abs(E[i:i + 1, :3] - math.pi * L.astype(np.float64)) <= etol).all() and (etol < 1e-3 * math.pi * L).all()


# ---- 8. sessions and refusals ------------------------------------------------------------------------------------
def test_a_call_leaves_everything_else_alone():
    sc = fl.scene_of(rc.combo_of("cornell+mesh"))
    pts, d, w, ps, ds = pc.probe_set()
    want = pc.oracle_records("cornell+mesh", 130, 2)
    state = {}
    for query in (False, True):
        q = VRendererHIP(0)
        scenes.load_into(q, sc)
        q.set_service(1)
        q.render(frames=2, times=[11, 12], sync=False)
        if query:
            s0 = q.service_info()["sessions"]
            same(probe(q, pts, d[:130], pc.weights_for(130), ps, ds[:130]), want, "inside a session")
        q.render(frames=2, times=[13, 14], sync=False)
        q.sync()
        if query:
            assert q.service_info()["sessions"] > s0 >= 1     # the call closed the first session
        state[query] = (q.read_accum(), q.read_rgba8(), q.read_depth8(), q.getFrameCount(), q.export_mesh_flat())
        q.cleanUp()
    for x, y in zip(state[False][:3], state[True][:3]):
        assert x.tobytes() == y.tobytes()
    assert state[False][3] == state[True][3] == 4
    assert all(state[False][4][k].tobytes() == state[True][4][k].tobytes() for k in state[False][4])


def test_refusals():
    import torch
    pts, d, w, ps, ds = (dev(a, t) for a, t in zip(pc.probe_set(), (np.float32,) * 3 + (np.uint32,) * 2))
    q = VRendererHIP([0])                                    # a multi-device context of one device
    q.init(64, 48)
    with pytest.raises(VRHIPError) as e:
        q.probeSH(pts, d, w, ps, ds)
    assert e.value.code == -1 and "multi-device" in str(e.value)
    with pytest.raises(VRHIPError) as e:
        q.shIrradiance(torch.zeros((4, 28), device="cuda:0"), torch.zeros((4, 3), device="cuda:0"))
    assert e.value.code == -1 and "multi-device" in str(e.value)
    q.cleanUp()
    q = fresh()                                              # HDRI mode, no environment
    with pytest.raises(VRHIPError) as e:
        q.probeSH(pts, d, w, ps, ds)
    assert e.value.code == -3
    assert tuple(q.probeSH(pts[:0], d, w, ps[:0], ds).shape) == (0, 28)        # nothing to do comes first
    q.useCornellBox(True)                                    # a scene without a mesh
    want = q.probeSH(pts, d, w, ps, ds).cpu().numpy()
    assert np.isfinite(want[:, :27]).all() and np.any(want[:, :27] != 0)
    for samples in (0, 4097):
        with pytest.raises(VRHIPError) as e:
            q.probeSH(pts, d, w, ps, ds, samples=samples)
        assert e.value.code == -1
    p = lambda x: ctypes.c_void_p(x.data_ptr())               # noqa: E731
    n, k = len(pts), len(d)
    out = torch.zeros((n + 1, 28), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    call = q._lib.vrhip_probe_sh
    assert call(q._ctx, p(pts), p(d), p(w), p(ps), p(ds), n, k, 2, ctypes.c_void_p(out.data_ptr() + 4)) == -1
    assert call(q._ctx, None, p(d), p(w), p(ps), p(ds), n, k, 2, p(out)) == -1
    assert call(q._ctx, p(pts), None, p(w), p(ps), p(ds), n, k, 2, p(out)) == -1
    assert call(q._ctx, p(pts), p(d), p(w), None, p(ds), n, k, 2, p(out)) == -1
    assert call(q._ctx, p(pts), p(d), p(w), p(ps), None, n, k, 2, p(out)) == -1
    assert call(q._ctx, p(pts), p(d), p(w), p(ps), p(ds), n, k, 2, None) == -1
    assert call(q._ctx, p(pts), p(d), p(w), p(ps), p(ds), n, 0, 2, p(out)) == -1
    assert call(q._ctx, p(pts), p(d), p(w), p(ps), p(ds), n, 65537, 2, p(out)) == -1
    assert not out.cpu().numpy().any()
    assert call(q._ctx, None, None, None, None, None, 0, 1, 2, None) == 0
    assert call(q._ctx, p(pts), p(d), None, p(ps), p(ds), n, k, 2, p(out)) == 0       # only the weights may be null
    wrong = [dict(points=pts.cpu(), dirs=d), dict(points=pts, dirs=d.double()), dict(points=pts[:, :2].contiguous(), dirs=d),
             dict(points=pts, dirs=d, weights=w[:-1]), dict(points=pts, dirs=d, weights=w[:, None]),
             dict(points=pts, dirs=d, probe_seeds=ps[:-1]), dict(points=pts, dirs=d, dir_seeds=ds[:-1]),
             dict(points=pts, dirs=d, dir_seeds=ds.float()), dict(points=pts, dirs=d, probe_seeds=ps.cpu()),
             dict(points=None, dirs=d), dict(points=pts, dirs=None)]
    for kw in wrong:                                         # device, dtype, shape, missing
        with pytest.raises(ValueError):
            q.probeSH(**kw)
    drawn = q.probeSH(pts, d, samples=4)                     # seeds drawn on the device
    assert tuple(drawn.shape) == (n, 28) and np.isfinite(drawn.cpu().numpy()[:, :27]).all()
    again = q.probeSH(pts, d, w, ps, ds).cpu().numpy()
    assert (pc.u32(again) == pc.u32(want)).all()
    assert q.probeSH(pts[:2], d[:3], None, ps[:2], ds[:3], samples=4096).shape[0] == 2       # the upper bound itself
    q.cleanUp()
